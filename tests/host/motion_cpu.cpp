// heatray_amd/csrc/hr_motion.h on the CPU (tests/test_motion_ref.py): the motion planes from given hits, the merge and the motion vectors,
// with the per-pixel functions the kernels compile and the host's camera arithmetic.  Input: int32 W, H, max_history, snapshot
// triangles, current meshes, 0, 0, 0; float normal_cos, plane_tol, min_weight, 0; the old camera (16 floats view matrix, aspect,
// fov_tan), the new camera likewise; the history (H0, H1, H2: W x H float4 each); the new view's frame, ALBEDO, NORMAL_DEPTH, MOMENTS;
// the hit of every pixel's centre ray (int32 prim or -1, float t, u, v); per current mesh (uint32 first triangle, int32 first triangle in
// the snapshot or -1); the snapshot (12 floats per triangle).  Output: Mv0, Mv1; uint64 surface, sky, unmatched; the merged frame,
// ALBEDO, NORMAL_DEPTH, MOMENTS; uint64 reused, rejected, samples; the motion vectors.
#include "hr_motion.h"

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

struct Hit {
    int32_t prim;
    float t, u, v;
};
struct Mesh {
    uint32_t triOffset;
    int32_t first;
};

template <class T> static bool readAll(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[8];
    float fl[4], camOld[18], camNew[18];
    if (fread(hd, 4, 8, f) != 8 || fread(fl, 4, 4, f) != 4 || fread(camOld, 4, 18, f) != 18 || fread(camNew, 4, 18, f) != 18) return 4;
    const int W = hd[0], H = hd[1], nTris = hd[3], nMeshes = hd[4];
    const size_t n = (size_t)W * H;
    std::vector<dn4> hist, in[4];
    std::vector<Hit> hits;
    std::vector<Mesh> meshes;
    std::vector<float> snap;
    if (!readAll(f, hist, 3 * n)) return 5;
    for (auto &v : in)
        if (!readAll(f, v, n)) return 5;
    if (!readAll(f, hits, n) || !readAll(f, meshes, (size_t)nMeshes) || !readAll(f, snap, (size_t)nTris * 12)) return 5;
    fclose(f);
    // ---- the trace's resolve (k_motion_trace behind the walk)
    std::vector<dn4> mv(2 * n), vec(n);
    uint64_t tr[3] = {0, 0, 0}, res[3] = {0, 0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            v3 o, d;
            mvCameraRay(camNew, camNew[16], camNew[17], x, y, (float)W, (float)H, o, d);
            dn4 &Mv0 = mv[i], &Mv1 = mv[n + i];
            mvMiss(Mv0, Mv1);
            const Hit &h = hits[i];
            if (h.prim < 0) {
                tr[1] += 1;
                continue;
            }
            float depth;
            const v3 Pw = mvHitPoint(o, d, h.t, v3(camNew[8], camNew[9], camNew[10]), depth);
            int lo = 0, hi = nMeshes - 1;
            while (lo < hi) {
                const int m = (lo + hi + 1) >> 1;
                if (meshes[m].triOffset <= (uint32_t)h.prim)
                    lo = m;
                else
                    hi = m - 1;
            }
            if (meshes[lo].first >= 0) {
                const float *t = snap.data() + 12 * ((size_t)meshes[lo].first + ((uint32_t)h.prim - meshes[lo].triOffset));
                mvMatched(v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8]), h.u, h.v, depth, Mv0, Mv1);
                tr[0] += 1;
            } else {
                mvUnmatched(Pw, depth, Mv0, Mv1);
                tr[2] += 1;
            }
        }
    // ---- the merge and the vectors
    const MvCam cam = mvCameras(camOld, camOld[16], camOld[17], camNew, camNew[16], camNew[17]);
    const HsParams P{(float)hd[2], fl[0], fl[1], fl[2]};
    const Vec src{hist, n};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            float nh = 0.0f;
            const int st = mvMerge(src, cam, P, mv[i], mv[n + i], x, y, W, H, in[0][i], in[1][i], in[2][i], in[3][i], &nh);
            if (st == HS_REUSED) res[0] += 1, res[2] += hsCount(nh);
            if (st == HS_REJECTED) res[1] += 1;
            vec[i] = mvVector(cam, mv[i], x, y, W, H);
        }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(mv.data(), sizeof(dn4), 2 * n, f) != 2 * n || fwrite(tr, 8, 3, f) != 3) return 6;
    for (auto &v : in)
        if (fwrite(v.data(), sizeof(dn4), n, f) != n) return 6;
    if (fwrite(res, 8, 3, f) != 3 || fwrite(vec.data(), sizeof(dn4), n, f) != n) return 6;
    fclose(f);
    printf("motion cpu: ok\n");
    return 0;
}
