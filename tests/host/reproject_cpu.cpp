// heatray_amd/csrc/hr_reproject.h on the CPU (tests/test_reproject_ref.py): capture a history from one frame, preview another frame from it,
// and merge it progressively into that frame, with the per-pixel functions the kernels compile and the host's camera arithmetic.
// Input: int32 W, H, max_history, 0; float normal_cos, plane_tol, min_weight, 0; the old camera (16 floats view matrix, aspect, fov_tan),
// the new camera likewise; the old frame, ALBEDO, NORMAL_DEPTH, MOMENTS (W x H float4 each); the new view's four likewise; the examined
// bits before the merge (W x H bytes, 0 / 1).  Output: the history (H0, H1, H2 planes); the preview of the new view's frame as it came
// in; the merged frame, ALBEDO, NORMAL_DEPTH, MOMENTS; the examined bytes after the merge; uint64 reused, rejected, samples, pending,
// examined; uint64 own, previewed, empty.
#include "hr_reproject.h"

#include <cstdio>
#include <vector>

using namespace hr;

struct Vec {
    const std::vector<dn4> &h;
    size_t n;
    dn4 h0(int i) const { return h[i]; }
    dn4 h1(int i) const { return h[n + i]; }
    dn4 h2(int i) const { return h[2 * n + i]; }
};

// the guide records straight from the frame and the planes (the kernel stages the same function's answers in LDS)
struct Guides {
    const std::vector<dn4> &F, &A, &G;
    int W;
    int cls(int gx, int gy) const
    {
        dn4 r;
        const size_t i = (size_t)gy * W + gx;
        return rpGuide(F[i].w, A[i], G[i], r);
    }
    dn4 rec(int gx, int gy) const
    {
        dn4 r;
        const size_t i = (size_t)gy * W + gx;
        rpGuide(F[i].w, A[i], G[i], r);
        return r;
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[4];
    float fl[4], camOld[18], camNew[18];
    if (fread(hd, 4, 4, f) != 4 || fread(fl, 4, 4, f) != 4 || fread(camOld, 4, 18, f) != 18 || fread(camNew, 4, 18, f) != 18) return 4;
    const int W = hd[0], H = hd[1];
    const size_t n = (size_t)W * H;
    std::vector<dn4> in[8];
    for (auto &v : in) {
        v.resize(n);
        if (fread(v.data(), sizeof(dn4), n, f) != n) return 5;
    }
    std::vector<uint8_t> E(n);
    if (fread(E.data(), 1, n, f) != n) return 5;
    fclose(f);
    std::vector<dn4> hist(3 * n);
    for (size_t i = 0; i < n; ++i) hsCapture(in[0][i], in[1][i], in[2][i], in[3][i], hist[i], hist[n + i], hist[2 * n + i]);
    const HsCam cam = hsCameras(camOld, camOld[16], camOld[17], camNew, camNew[16], camNew[17]);
    const HsParams P{(float)hd[2], fl[0], fl[1], fl[2]};
    const Vec src{hist, n};

    std::vector<dn4> preview(n);
    uint64_t pres[3] = {0, 0, 0};
    {
        const Guides guides{in[4], in[5], in[6], W};
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                if (in[4][i].w > 0.0f) {
                    preview[i] = rpOwn(in[4][i]);
                    pres[RP_OWN] += 1;
                    continue;
                }
                int gx, gy;
                dn4 rec;
                const int cls = rpFindGuide(guides, x, y, W, H, gx, gy, rec);
                pres[rpPreviewFromGuide(src, cam, P, x, y, W, H, cls, gx, gy, rec, preview[i])] += 1;
            }
    }

    uint64_t res[5] = {0, 0, 0, 0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            if (!E[i] && in[4][i].w > 0.0f) {
                float nh = 0.0f;
                const int st = hsMerge(src, cam, P, x, y, W, H, in[4][i], in[5][i], in[6][i], in[7][i], &nh);
                if (st == HS_REUSED) res[0] += 1, res[2] += hsCount(nh);
                if (st == HS_REJECTED) res[1] += 1;
                E[i] = 1;
            }
            res[E[i] ? 4 : 3] += 1;
        }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(hist.data(), sizeof(dn4), 3 * n, f) != 3 * n) return 6;
    if (fwrite(preview.data(), sizeof(dn4), n, f) != n) return 6;
    for (int k = 4; k < 8; ++k)
        if (fwrite(in[k].data(), sizeof(dn4), n, f) != n) return 6;
    if (fwrite(E.data(), 1, n, f) != n) return 6;
    if (fwrite(res, 8, 5, f) != 5 || fwrite(pres, 8, 3, f) != 3) return 6;
    fclose(f);
    printf("reproject cpu: ok\n");
    return 0;
}
