// heatray_amd/csrc/hr_exposure.h on the CPU (tests/test_exposure_ref.py, also built with -fsanitize=address,undefined): the bins and the
// class counters of an image read from a file, or bins given as they are, then the ordered reduce, with the functions the kernels compile.
// Input: int32 mode (0: an image follows, 1: 256 uint64 bins follow), W, H, hasState; int32 window x0 y0 x1 y1 (all 0: the whole image);
// int32 low_permille, high_permille; float key, min_scale, max_scale, adapt, prev (the state's scale).  Output: 256 uint64 bins; uint64
// below, above, nonfinite, invalid; float scale, target, key_luminance; uint32 position; uint64 counted, used; uint32 flags, 1 when there
// is a state afterwards; float its scale.
#include "hr_exposure.h"

#include <cstdio>
#include <vector>

using namespace hr;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[10];
    float fl[5];
    if (fread(hd, 4, 10, f) != 10 || fread(fl, 4, 5, f) != 5) return 4;
    const int mode = hd[0], W = hd[1], H = hd[2];
    std::vector<unsigned long long> words(kExWords, 0ull);
    if (mode == 0) {
        const size_t n = (size_t)W * H;
        std::vector<dn4> image(n);
        if (fread(image.data(), sizeof(dn4), n, f) != n) return 5;
        ExWindow win{hd[4], hd[5], hd[6], hd[7]};
        if (win.x0 == 0 && win.y0 == 0 && win.x1 == 0 && win.y1 == 0) win = ExWindow{0, 0, W, H};
        for (int y = win.y0; y < win.y1; ++y)
            for (int x = win.x0; x < win.x1; ++x) words[exClass(image[(size_t)y * W + x])] += 1;
    } else if (fread(words.data(), 8, kExBins, f) != (size_t)kExBins) {
        return 5;
    }
    fclose(f);
    const ExParams P{fl[0], hd[8], hd[9], fl[1], fl[2], fl[3]};
    ExReduced r;
    float next = 0.0f;
    const bool has = exReduce(words.data(), P, hd[3] != 0, fl[4], r, &next);
    const uint32_t hasWord = has ? 1u : 0u;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(words.data(), 8, kExBins + 4, f) != (size_t)kExBins + 4 || fwrite(&r.scale, 4, 1, f) != 1 || fwrite(&r.target, 4, 1, f) != 1 ||
        fwrite(&r.lavg, 4, 1, f) != 1 || fwrite(&r.position, 4, 1, f) != 1 || fwrite(&r.counted, 8, 1, f) != 1 || fwrite(&r.used, 8, 1, f) != 1 ||
        fwrite(&r.flags, 4, 1, f) != 1 || fwrite(&hasWord, 4, 1, f) != 1 || fwrite(&next, 4, 1, f) != 1)
        return 6;
    fclose(f);
    printf("exposure cpu: ok\n");
    return 0;
}
