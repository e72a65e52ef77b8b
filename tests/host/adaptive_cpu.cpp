// heatray_amd/csrc/hr_adaptive.h on the CPU (tests/test_adaptive_ref.py): the error map and the sample mask of a frame read from a file,
// with the per-pixel functions the kernels compile; the dilation is the contract's sentence, by brute force.  Input: int32 W, H,
// min_samples, radius; float threshold, floor; then frame and MOMENTS (W x H float4 each).  Output: W x H floats (the error map), then
// W x H bytes (the mask), then uint64 unconverged, uint64 active, uint32 bits of the largest finite error.
#include "hr_adaptive.h"

#include <cstdio>
#include <vector>

using namespace hr;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[4];
    float fl[2];
    if (fread(hd, 4, 4, f) != 4 || fread(fl, 4, 2, f) != 2) return 4;
    const int W = hd[0], H = hd[1], radius = hd[3];
    const size_t n = (size_t)W * H;
    std::vector<dn4> frame(n), moments(n);
    if (fread(frame.data(), sizeof(dn4), n, f) != n || fread(moments.data(), sizeof(dn4), n, f) != n) return 5;
    fclose(f);
    std::vector<float> err(n);
    std::vector<uint8_t> mask(n);
    uint64_t unconverged = 0, active = 0;
    uint32_t maxBits = 0;
    for (size_t i = 0; i < n; ++i) {
        err[i] = adError(frame[i], moments[i], fl[1], (float)hd[2]);
        unconverged += adUnconverged(err[i], fl[0]) ? 1 : 0;
        const uint32_t b = adFiniteBits(err[i]);
        maxBits = b > maxBits ? b : maxBits;
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool on = false;
            for (int qy = y - radius; qy <= y + radius; ++qy)
                for (int qx = x - radius; qx <= x + radius; ++qx)
                    if (qx >= 0 && qx < W && qy >= 0 && qy < H && adUnconverged(err[(size_t)qy * W + qx], fl[0])) on = true;
            mask[(size_t)y * W + x] = on ? 1 : 0;
            active += on ? 1 : 0;
        }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(err.data(), 4, n, f) != n || fwrite(mask.data(), 1, n, f) != n || fwrite(&unconverged, 8, 1, f) != 1 || fwrite(&active, 8, 1, f) != 1 ||
        fwrite(&maxBits, 4, 1, f) != 1)
        return 6;
    fclose(f);
    printf("adaptive cpu: ok\n");
    return 0;
}
