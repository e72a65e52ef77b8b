// hrcore_group_stub.cpp — TEST INFRASTRUCTURE.  The context-group entry points of include/hrcore_group.h for the CPU-only sanitizer
// runs of the C++ drop-in layer, beside the do-nothing stub of include/hrcore.h (tests/host/hrcore_stub.cpp).  A "group" here is one
// stub context (it renders nothing) plus the member devices it was asked for, so that PassGenerator's HEATRAY_DEVICES path — parse,
// create, report the members, every later call on the group handle, destroy — runs under ThreadSanitizer / AddressSanitizer.  Linked
// ONLY into that test executable, never part of libheatrayhost or the product.
#include "hrcore_group.h"

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace {
std::mutex g_mutex;
std::map<const hr_ctx *, std::vector<int32_t>> g_groups; // group handle -> member devices
const int kStubDevices = 1;                              // "every visible device": the stub sees one
} // namespace

extern "C" {
uint32_t hr_group_api_version(void) { return HR_GROUP_API_VERSION; }

int hr_ctx_create_group(const hr_ctx_desc *desc, const int32_t *device_ids, int32_t n, hr_ctx **out)
{
    if (!out) return HR_ERR_INVALID;
    *out = nullptr;
    if ((desc && (desc->rank != 0 || desc->world > 1)) || n < 0 || n > HR_GROUP_MAX_MEMBERS || (n > 0 && !device_ids)) return HR_ERR_INVALID;
    std::vector<int32_t> ids;
    for (int i = 0; i < (n > 0 ? n : kStubDevices); ++i) {
        const int32_t d = n > 0 ? device_ids[i] : i;
        if (d < 0 || d >= kStubDevices) return HR_ERR_INVALID;
        ids.push_back(d);
    }
    const int rc = hr_ctx_create(desc, out);
    if (rc != HR_OK) return rc;
    std::lock_guard<std::mutex> lock(g_mutex);
    g_groups[*out] = ids;
    return HR_OK;
}

int hr_group_get_info(hr_ctx *group, hr_group_info *out)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_groups.find(group);
    if (it == g_groups.end() || !out) return HR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->n_members = (int32_t)it->second.size();
    for (size_t i = 0; i < it->second.size(); ++i) out->device_ids[i] = it->second[i];
    return HR_OK;
}

int hr_group_member_stats(hr_ctx *group, int32_t member, hr_pass_stats *stats, hr_kernel_times *times)
{
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        auto it = g_groups.find(group);
        if (it == g_groups.end() || member < 0 || member >= (int32_t)it->second.size()) return HR_ERR_INVALID;
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (times) std::memset(times, 0, sizeof(*times));
    return HR_OK;
}
}
