// heatray_amd/csrc/hr_metric.h on the CPU (tests/test_metric_ref.py, also built with -fsanitize=address,undefined): the terms, bins and
// counters of two images read from a file, or bins given as they are, then the fold, with the functions the kernel and the library compile.
// Input: int32 mode (0: compare, two images follow: the image, the reference; 1: estimate, the frame and its MOMENTS plane follow; 2:
// 512 uint64 bins follow, NUM then DEN, then uint64 counted and uint64 kind), W, H; int32 window x0 y0 x1 y1 (all 0: the whole image).
// Output: the kMtWords uint64 words of a measurement (512 bins; counted, differing, nonfinite, skipped; the bits of max_abs); double num,
// den, value, mse; uint32 flags.
#include "hr_metric.h"

#include <cstdio>
#include <vector>

using namespace hr;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[7];
    if (fread(hd, 4, 7, f) != 7) return 4;
    const int mode = hd[0], W = hd[1], H = hd[2];
    std::vector<unsigned long long> words(kMtWords, 0ull);
    uint32_t kind = mode == 1 ? kMtEstimate : kMtCompare;
    if (mode == 2) {
        unsigned long long tail[2];
        if (fread(words.data(), 8, 2 * kMtBins, f) != (size_t)(2 * kMtBins) || fread(tail, 8, 2, f) != 2) return 5;
        words[kMtWordCounted] = tail[0], kind = (uint32_t)tail[1];
    } else {
        const size_t n = (size_t)W * H;
        std::vector<dn4> a(n), b(n);
        if (fread(a.data(), sizeof(dn4), n, f) != n || fread(b.data(), sizeof(dn4), n, f) != n) return 5;
        MtWindow win{hd[3], hd[4], hd[5], hd[6]};
        if (win.x0 == 0 && win.y0 == 0 && win.x1 == 0 && win.y1 == 0) win = MtWindow{0, 0, W, H};
        const auto add = [&words](int set, float t) { words[set + mtBin(t)] += mtMantissa(t); };
        for (int y = win.y0; y < win.y1; ++y)
            for (int x = win.x0; x < win.x1; ++x) {
                const size_t i = (size_t)y * W + x;
                int cls;
                if (mode == 0) {
                    float tx[3], ty[3];
                    bool differing;
                    uint32_t maxAbs;
                    cls = mtCompare(a[i], b[i], tx, ty, differing, maxAbs);
                    if (cls == kMtCounted) {
                        for (int k = 0; k < 3; ++k) add(kMtWordNum, tx[k]), add(kMtWordDen, ty[k]);
                        if (differing) words[kMtWordDiffering] += 1;
                        if (maxAbs > words[kMtWordMaxAbs]) words[kMtWordMaxAbs] = maxAbs;
                    }
                } else {
                    float tx, ty;
                    cls = mtEstimate(a[i], b[i], tx, ty);
                    if (cls == kMtCounted) add(kMtWordNum, tx), add(kMtWordDen, ty);
                }
                words[cls == kMtCounted ? kMtWordCounted : (cls == kMtNonfinite ? kMtWordNonfinite : kMtWordSkipped)] += 1;
            }
    }
    fclose(f);
    const MtFolded r = mtFinish(words.data(), kind);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(words.data(), 8, kMtWords, f) != (size_t)kMtWords || fwrite(&r.num, 8, 1, f) != 1 || fwrite(&r.den, 8, 1, f) != 1 || fwrite(&r.value, 8, 1, f) != 1 ||
        fwrite(&r.mse, 8, 1, f) != 1 || fwrite(&r.flags, 4, 1, f) != 1)
        return 6;
    fclose(f);
    printf("metric cpu: ok\n");
    return 0;
}
