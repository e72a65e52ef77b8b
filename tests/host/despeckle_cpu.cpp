// heatray_amd/csrc/hr_despeckle.h on the CPU (tests/test_despeckle_ref.py, also built with -fsanitize=address,undefined): the
// despeckled frame and moments and the five counters of a pair read from a file, with the functions the kernel compiles.
// Input: int32 W, H, rank, min_taps; float ratio, sigmas, floor, 0; the frame, then its MOMENTS plane (W x H float4 each).
// Output: the despeckled frame, the despeckled moments; uint64 valid, clamped, kept, starved, nonfinite pixels.
#include "hr_despeckle.h"

#include <cstdio>
#include <vector>

using namespace hr;

// the source dkPixel reads: dkClass's luminance of every pixel, as the kernel's LDS tile holds it
struct LumPlane {
    const float *l;
    int W;
    float lum(int x, int y) const { return l[(size_t)y * W + x]; }
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[4];
    float fl[4];
    if (fread(hd, 4, 4, f) != 4 || fread(fl, 4, 4, f) != 4) return 4;
    const int W = hd[0], H = hd[1];
    const DkParams P{hd[2], hd[3], fl[0], fl[1], fl[2]};
    const size_t n = (size_t)W * H;
    std::vector<dn4> frame(n), mom(n), out(n), mout(n);
    if (fread(frame.data(), sizeof(dn4), n, f) != n || fread(mom.data(), sizeof(dn4), n, f) != n) return 5;
    fclose(f);
    std::vector<float> lum(n);
    for (size_t i = 0; i < n; ++i) dkClass(frame[i], lum[i]);
    const LumPlane s{lum.data(), W};
    unsigned long long words[5] = {0, 0, 0, 0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            dn4 fp = frame[i], mp = mom[i];
            const int st = dkPixel(s, x, y, W, H, P, fp, mp);
            out[i] = fp, mout[i] = mp;
            if (st >= DK_PASSED) words[0] += 1;
            if (st == DK_CLAMPED) words[1] += 1;
            if (st == DK_KEPT) words[2] += 1;
            if (st == DK_STARVED) words[3] += 1;
            if (st == DK_NONFINITE) words[4] += 1;
        }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(dn4), n, f) != n || fwrite(mout.data(), sizeof(dn4), n, f) != n || fwrite(words, 8, 5, f) != 5) return 6;
    fclose(f);
    printf("despeckle cpu: ok\n");
    return 0;
}
