#pragma once
// HEATRAY_DEVICES: which devices one frame is split over (a context group, include/hrcore_group.h).
//   "all"        every visible device once
//   "0,1,2,3"    member i renders on the i-th listed device; ids may repeat ("0,0": two members share device 0)
// Anything else (empty items, signs, spaces, more than HR_GROUP_MAX_MEMBERS ids) is malformed: the caller fails loudly.

#include <hrcore_group.h>

#include <stdint.h>
#include <string>
#include <vector>

namespace heatray {

// true and the list (empty for "all") when `text` is well formed; false and a message otherwise
inline bool parseDeviceList(const char* text, std::vector<int32_t>& ids, std::string& error)
{
    ids.clear();
    const std::string s = text ? text : "";
    if (s == "all") return true;
    size_t i = 0;
    while (true) {
        if (i >= s.size() || s[i] < '0' || s[i] > '9') {
            error = "HEATRAY_DEVICES=\"" + s + "\": expected \"all\" or a comma-separated list of device ids such as 0,1,2,3";
            ids.clear();
            return false;
        }
        long long v = 0;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9' && v <= 1000000) v = v * 10 + (s[i++] - '0');
        if (v > 1000000 || (i < s.size() && s[i] != ',')) {
            error = "HEATRAY_DEVICES=\"" + s + "\": expected \"all\" or a comma-separated list of device ids such as 0,1,2,3";
            ids.clear();
            return false;
        }
        ids.push_back((int32_t)v);
        if ((int)ids.size() > HR_GROUP_MAX_MEMBERS) {
            error = "HEATRAY_DEVICES=\"" + s + "\": more than " + std::to_string(HR_GROUP_MAX_MEMBERS) + " members";
            ids.clear();
            return false;
        }
        if (i == s.size()) return true;
        ++i; // ','
    }
}

} // namespace heatray
