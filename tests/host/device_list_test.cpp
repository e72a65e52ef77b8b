// device_list_test.cpp — TEST INFRASTRUCTURE: the HEATRAY_DEVICES parser of the C++ layer (heatray_amd/host/HeatrayRenderer/DeviceList.h)
// on the command line, for tests/test_group_abi.py.  Prints "ok all", "ok <id> <id> ..." or "error <message>" for argv[1].
#include <HeatrayRenderer/DeviceList.h>

#include <cstdio>

int main(int argc, char** argv)
{
    std::vector<int32_t> ids;
    std::string error;
    if (!heatray::parseDeviceList(argc > 1 ? argv[1] : "", ids, error)) {
        printf("error %s\n", error.c_str());
        return 0;
    }
    printf("ok");
    if (ids.empty()) printf(" all");
    for (int32_t d : ids) printf(" %d", d);
    printf("\n");
    return 0;
}
