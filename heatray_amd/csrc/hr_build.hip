// hr_build.hip — scene assembly and BVH construction on the GPU (the table generators are in hr_tables.hip).
//
// Replaces what OpenRL does with the buffers of rlDrawElements (/root/reference/Source/HeatrayRenderer/
// Scene/Mesh.cpp:29-153, Resources/shaders/vertex.rlsl:25-43) — SURVEY §8a row a6.
//
//   assemble : one thread per triangle: world transform, edge form, shading attributes, scene bounds
//   morton   : 30-bit Morton code of the triangle-AABB centre, normalised by the scene bounds
//   sort     : LSD radix sort, 4 x 8-bit digits, stable (histogram / scan / ballot-ranked scatter)
//   karras   : binary radix tree over the sorted (key, index) pairs
//   refit    : bottom-up boxes and collapse costs in kernel-ordered rounds (no inter-workgroup hand-off inside a
//              launch, so no reliance on cross-XCD visibility)
//   sah      : the radix tree's bottom subtrees rebuilt by full-sweep SAH (hr_sah_subtree.h)
//   ploc     : the second candidate, by parallel locally-ordered clustering; the cheaper collapse is kept
//   collapse : the binary tree to 4-wide nodes by minimal summed node area; 64-byte nodes, then the 32-byte encode
#include "hr_kernels.h"
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace hr {

#define HR_CHECK(expr)                  \
    do {                                \
        hipError_t e_ = (expr);         \
        if (e_ != hipSuccess) return 1; \
    } while (0)

HRD uint32_t orderedFromFloat(float f)
{
    uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

HRD v3 fetch3(const float *a, uint32_t i, int stride) { const float *p = a + (size_t)i * stride; return v3(p[0], p[1], p[2]); }

// ------------------------------------------------------------------------------------- assemble
__global__ __launch_bounds__(256) void k_assemble(const GeomDev *__restrict__ geoms, int nGeoms, uint32_t nTris, Tri *__restrict__ tris,
                                                  const uint32_t *__restrict__ slotOfPrim, TriAttr *__restrict__ attrs,
                                                  TriAttrExt *__restrict__ ext, uint32_t *__restrict__ bounds)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    v3 lo(__builtin_inff()), hi(-__builtin_inff());
    if (t < nTris) {
        int a = 0, b = nGeoms - 1; // last geometry with triOffset <= t
        while (a < b) {
            int m = (a + b + 1) >> 1;
            if (geoms[m].triOffset <= t)
                a = m;
            else
                b = m - 1;
        }
        const GeomDev &g = geoms[a];
        const uint32_t lt = t - g.triOffset;
        uint32_t i0, i1, i2;
        if (g.strip) { // GL strip ordering: odd triangles swap the first two vertices
            i0 = g.idx[lt], i1 = g.idx[lt + 1], i2 = g.idx[lt + 2];
            if (lt & 1u) {
                uint32_t s = i0;
                i0 = i1;
                i1 = s;
            }
        } else {
            i0 = g.idx[3 * lt], i1 = g.idx[3 * lt + 1], i2 = g.idx[3 * lt + 2];
        }
        const uint32_t id[3] = {i0, i1, i2};
        // vertex.rlsl:27 — rl_Position = worldFromEntity * vec4(position, 1)
        const v3 p0 = xformPoint(g.world, fetch3(g.pos, i0, g.posStride)), p1 = xformPoint(g.world, fetch3(g.pos, i1, g.posStride)),
                 p2 = xformPoint(g.world, fetch3(g.pos, i2, g.posStride));
        const v3 e1 = p1 - p0, e2 = p2 - p0;
        Tri tr;
        tr.p = make_float4(p0.x, p0.y, p0.z, e1.x);
        tr.q = make_float4(e1.y, e1.z, e2.x, e2.y);
        tr.r = make_float4(e2.z, __uint_as_float(t), __uint_as_float(g.flags), 0.0f);
        tris[slotOfPrim ? slotOfPrim[t] : t] = tr;
        TriAttr at;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // vertex.rlsl:28-29 — normal = mat3(worldFromEntity) * normalAttribute
            const v3 n = xformVector(g.world, fetch3(g.nrm, id[k], g.nrmStride));
            at.n[3 * k] = n.x, at.n[3 * k + 1] = n.y, at.n[3 * k + 2] = n.z;
            at.uv[2 * k] = g.uv ? g.uv[(size_t)id[k] * g.uvStride] : 0.0f;
            at.uv[2 * k + 1] = g.uv ? g.uv[(size_t)id[k] * g.uvStride + 1] : 0.0f;
        }
        at.matflags = (g.material & kMatMask) | (g.flags << 24);
        attrs[t] = at;
        if (ext) {
            TriAttrExt e;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v3 tn(0.0f), bt(0.0f), cl(0.0f);
                if (g.tan && g.bit) { // vertex.rlsl:35-38
                    tn = xformVector(g.world, fetch3(g.tan, id[k], g.tanStride));
                    bt = xformVector(g.world, fetch3(g.bit, id[k], g.bitStride));
                }
                if (g.col) cl = fetch3(g.col, id[k], g.colStride); // vertex.rlsl:40-42
                e.tan[3 * k] = tn.x, e.tan[3 * k + 1] = tn.y, e.tan[3 * k + 2] = tn.z;
                e.bit[3 * k] = bt.x, e.bit[3 * k + 1] = bt.y, e.bit[3 * k + 2] = bt.z;
                e.col[3 * k] = cl.x, e.col[3 * k + 1] = cl.y, e.col[3 * k + 2] = cl.z;
            }
            e.pad = 0.0f;
            ext[t] = e;
        }
        // bounds over v0, v0+e1, v0+e2 (the vertices the intersector sees)
        const v3 q1 = p0 + e1, q2 = p0 + e2;
        lo = min3(min3(p0, q1), q2);
        hi = max3(max3(p0, q1), q2);
    }
    // wave reduction, then block reduction through LDS, then one atomic per workgroup and component into one of kBoundSlots copies
    // of the bounds (same-address atomics serialise: one per wave into a single copy cost 0.9 ms for a million triangles)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo.x = fmin_(lo.x, __shfl_xor(lo.x, o)), lo.y = fmin_(lo.y, __shfl_xor(lo.y, o)), lo.z = fmin_(lo.z, __shfl_xor(lo.z, o));
        hi.x = fmax_(hi.x, __shfl_xor(hi.x, o)), hi.y = fmax_(hi.y, __shfl_xor(hi.y, o)), hi.z = fmax_(hi.z, __shfl_xor(hi.z, o));
    }
    __shared__ float red[4][6];
    if ((threadIdx.x & 63) == 0) {
        float *r = red[threadIdx.x >> 6];
        r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = hi.x, r[4] = hi.y, r[5] = hi.z;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float v = red[0][k];
        for (int w = 1; w < 4; ++w) v = k < 3 ? fmin_(v, red[w][k]) : fmax_(v, red[w][k]);
        uint32_t *slot = bounds + 6 * (blockIdx.x & (kBoundSlots - 1));
        if (k < 3) {
            if (v != __builtin_inff()) atomicMin(&slot[k], orderedFromFloat(v));
        } else {
            if (v != -__builtin_inff()) atomicMax(&slot[k], orderedFromFloat(v));
        }
    }
}

__global__ void k_bounds_init(uint32_t *bounds)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6 * kBoundSlots) bounds[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

void launchAssemble(hipStream_t st, const GeomDev *geoms, int nGeoms, uint32_t nTris, Tri *tris, const uint32_t *slotOfPrim, TriAttr *attrs,
                    TriAttrExt *ext, uint32_t *bounds)
{
    if (nTris == 0) return;
    hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(6 * kBoundSlots), 0, st, bounds);
    hipLaunchKernelGGL(k_assemble, dim3((nTris + 255) / 256), dim3(256), 0, st, geoms, nGeoms, nTris, tris, slotOfPrim, attrs, ext, bounds);
}

HRD float floatFromOrderedDev(uint32_t u)
{
    const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    return __uint_as_float(b);
}
__global__ void k_scene_consts(const uint32_t *__restrict__ bounds, SceneConsts *__restrict__ out, SceneDev *__restrict__ scene)
{
    SceneConsts c;
    for (int k = 0; k < 3; ++k) {
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        for (int sl = 0; sl < kBoundSlots; ++sl) {
            const uint32_t a = bounds[6 * sl + k], b = bounds[6 * sl + 3 + k];
            lo = a < lo ? a : lo, hi = b > hi ? b : hi;
        }
        c.lo[k] = floatFromOrderedDev(lo), c.hi[k] = floatFromOrderedDev(hi);
    }
    // |hi - lo| with the contract's operation order: sqrt((x*x + y*y) + z*z), correctly rounded like the host's sqrtf
    const float ex = c.hi[0] - c.lo[0], ey = c.hi[1] - c.lo[1], ez = c.hi[2] - c.lo[2];
    c.diag = sqrt_(ex * ex + ey * ey + ez * ez);
    c.pad = 1e-5f * c.diag;
    c.eps = 1e-4f * c.diag;
    c.areaSum = 0.0f, c.triAreaSum = 0.0f, c.pad1 = 0u;
    *out = c;
    if (scene) scene->rayEps = c.eps, scene->hitPad = 0.5f * c.pad;
}
void launchSceneConsts(hipStream_t st, const uint32_t *bounds, SceneConsts *out, SceneDev *scene)
{
    hipLaunchKernelGGL(k_scene_consts, dim3(1), dim3(1), 0, st, bounds, out, scene);
}

// --------------------------------------------------------------------------------------- morton
HRD uint32_t expandBits10(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
HRD uint32_t quantize10(float c, float lo, float ext)
{
    float q = (ext > 0.0f) ? (c - lo) / ext : 0.0f;
    q = q * 1024.0f;
    q = fmin_(fmax_(q, 0.0f), 1023.0f);
    return (uint32_t)q;
}
HRD void triBounds(const Tri &t, v3 &bl, v3 &bh)
{
    const v3 v0(t.p.x, t.p.y, t.p.z), e1(t.p.w, t.q.x, t.q.y), e2(t.q.z, t.q.w, t.r.x);
    const v3 p1 = v0 + e1, p2 = v0 + e2;
    bl = min3(min3(v0, p1), p2);
    bh = max3(max3(v0, p1), p2);
}

__global__ __launch_bounds__(256) void k_morton(const Tri *__restrict__ tris, uint32_t n, v3 lo, v3 ext, uint32_t *__restrict__ keys,
                                                uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    v3 bl, bh;
    triBounds(tris[i], bl, bh);
    const v3 c = (bl + bh) * 0.5f;
    keys[i] = (expandBits10(quantize10(c.x, lo.x, ext.x)) << 2) | (expandBits10(quantize10(c.y, lo.y, ext.y)) << 1) |
              expandBits10(quantize10(c.z, lo.z, ext.z));
    vals[i] = i;
}

// ----------------------------------------------------------------------------------- radix sort
static const int kSortTile = 2048; // keys per single-wave workgroup

__global__ __launch_bounds__(64) void k_sort_hist(const uint32_t *__restrict__ keys, uint32_t n, int shift, uint32_t *__restrict__ blockHist,
                                                  uint32_t nBlocks)
{
    __shared__ uint32_t hist[256];
    for (int i = threadIdx.x; i < 256; i += 64) hist[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (int r = 0; r < kSortTile / 64; ++r) {
        const uint32_t i = base + r * 64 + threadIdx.x;
        if (i < n) atomicAdd(&hist[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += 64) blockHist[(uint32_t)i * nBlocks + blockIdx.x] = hist[i];
}

// exclusive scan of `n` values by ONE workgroup of 1024 threads (n is at most a few hundred thousand)
__global__ __launch_bounds__(1024) void k_scan_single(uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ total)
{
    __shared__ uint32_t waveSums[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = (i < n) ? data[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t t = __shfl_up(inc, o);
            if ((int)lane >= o) inc += t;
        }
        if (lane == 63) waveSums[wave] = inc;
        __syncthreads();
        uint32_t wavePrefix = 0;
        for (uint32_t w = 0; w < wave; ++w) wavePrefix += waveSums[w];
        const uint32_t c = carry;
        if (i < n) data[i] = c + wavePrefix + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + wavePrefix + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) *total = carry;
}

__global__ __launch_bounds__(64) void k_sort_scatter(const uint32_t *__restrict__ keysIn, const uint32_t *__restrict__ valsIn, uint32_t n, int shift,
                                                     const uint32_t *__restrict__ blockOffsets, uint32_t nBlocks, uint32_t *__restrict__ keysOut,
                                                     uint32_t *__restrict__ valsOut)
{
    __shared__ uint32_t off[256];
    for (int i = threadIdx.x; i < 256; i += 64) off[i] = blockOffsets[(uint32_t)i * nBlocks + blockIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x;
    const unsigned long long ltMask = (1ull << lane) - 1ull;
    const uint32_t base = blockIdx.x * kSortTile;
    for (int r = 0; r < kSortTile / 64; ++r) {
        const uint32_t i = base + r * 64 + lane;
        const bool valid = i < n;
        const uint32_t key = valid ? keysIn[i] : 0u, val = valid ? valsIn[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        // lanes holding the same digit (stable: rank = number of equal-digit lanes before me)
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        uint32_t pos = 0;
        if (valid) pos = off[d] + (uint32_t)__popcll(same & ltMask);
        __syncthreads();
        if (valid && (same & ltMask) == 0ull) off[d] += (uint32_t)__popcll(same); // first lane of each digit group
        __syncthreads();
        if (valid) {
            keysOut[pos] = key;
            valsOut[pos] = val;
        }
    }
}

__global__ __launch_bounds__(256) void k_gather_tris(const Tri *__restrict__ trisPrim, const uint32_t *__restrict__ order, uint32_t n,
                                                     Tri *__restrict__ sorted, float pad, Box6 *__restrict__ leafBox)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Tri t = trisPrim[order[i]];
    sorted[i] = t;
    v3 bl, bh;
    triBounds(t, bl, bh);
    Box6 b;
    b.lo[0] = bl.x - pad, b.lo[1] = bl.y - pad, b.lo[2] = bl.z - pad;
    b.hi[0] = bh.x + pad, b.hi[1] = bh.y + pad, b.hi[2] = bh.z + pad;
    leafBox[i] = b;
}

// --------------------------------------------------------------------------------------- karras
HRD int deltaKey(const uint32_t *keys, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    const uint32_t a = keys[i], b = keys[j];
    if (a == b) return 32 + __clz((int)((uint32_t)i ^ (uint32_t)j));
    return __clz((int)(a ^ b));
}

#include "hr_sah_subtree.h"
struct KNode {
    int left, right; // >= 0: internal node, < 0: leaf ~index
    int first, last; // covered range of sorted triangles
};

__global__ __launch_bounds__(256) void k_karras(const uint32_t *__restrict__ keys, int n, KNode *__restrict__ nodes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (deltaKey(keys, n, i, i + 1) - deltaKey(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = deltaKey(keys, n, i, i - d);
    int lmax = 2;
    while (deltaKey(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (deltaKey(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = deltaKey(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (deltaKey(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    KNode k;
    k.left = (lo == gamma) ? ~gamma : gamma;
    k.right = (hi == gamma + 1) ? ~(gamma + 1) : gamma + 1;
    k.first = lo, k.last = hi;
    nodes[i] = k;
}

HRD float boxArea(const Box6 &b)
{
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// (C1, C2, C3, C4) of a binary node from its children's (see k_refit_round); a triangle child (ref < 0) costs nothing
HRD float4 collapseCost(int left, int right, float area, const float4 *__restrict__ cost)
{
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 cl = left < 0 ? z : cost[left], cr = right < 0 ? z : cost[right];
    const float h2 = cl.x + cr.x;
    const float h3 = fmin_(cl.x + cr.y, cl.y + cr.x);
    const float h4 = fmin_(cl.x + cr.z, fmin_(cl.y + cr.y, cl.z + cr.x));
    const float c1 = area + h4;
    const float c2 = fmin_(c1, h2), c3 = fmin_(c2, h3), c4 = fmin_(c3, h4);
    return make_float4(c1, c2, c3, c4);
}

// One bottom-up round: a node whose children were finished in an EARLIER launch gets its box.
// stamp[i] = round in which node i was finished (0 = not yet); visibility comes from the kernel boundary.
// ... and the costs of the collapse to a 4-wide tree (k_collapse4): cost[i] = (C1, C2, C3, C4), Ck = the least sum of the surface areas of
// the 4-wide nodes that can represent the subtree of binary node i when it may occupy up to k child slots of its 4-wide parent
// (k = 1: it is a child itself, a node of its own; k >= 2: it may be opened and its two children share the slots).  A triangle costs
// nothing: it is a child slot wherever it ends up.  Surface area = the probability that a ray visits the node (SAH).
__global__ __launch_bounds__(256) void k_refit_round(const KNode *__restrict__ nodes, int nInternal, const Box6 *__restrict__ leafBox,
                                                     Box6 *__restrict__ nodeBox, uint32_t *__restrict__ stamp, uint32_t round, float4 *__restrict__ cost)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nInternal || stamp[i] != 0u) return;
    const KNode k = nodes[i];
    const bool lr = k.left < 0 || (stamp[k.left] != 0u && stamp[k.left] < round);
    const bool rr = k.right < 0 || (stamp[k.right] != 0u && stamp[k.right] < round);
    if (!(lr && rr)) return;
    const Box6 a = k.left < 0 ? leafBox[~k.left] : nodeBox[k.left];
    const Box6 b = k.right < 0 ? leafBox[~k.right] : nodeBox[k.right];
    Box6 u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u.lo[c] = fmin_(a.lo[c], b.lo[c]);
        u.hi[c] = fmax_(a.hi[c], b.hi[c]);
    }
    nodeBox[i] = u;
    cost[i] = collapseCost(k.left, k.right, boxArea(u), cost);
    stamp[i] = round;
}

// biased exponent e (1..254) of the smallest power of two s = 2^(e-127) with ext / s <= 255
HRD uint32_t quantExponent(float ext)
{
    const float f = ext * (1.0f / 255.0f);
    uint32_t bits = __float_as_uint(f);
    uint32_t e = (bits >> 23) & 0xFFu;
    if (bits & 0x007FFFFFu) e += 1;                   // round the scale up to a power of two
    if (__uint_as_float(e << 23) * 255.0f < ext) e += 1; // guard against the rounding of ext/255
    return e < 1u ? 1u : (e > 254u ? 254u : e);
}

// Quantise the child boxes of a node against the node's own box (origin + q * 2^e, 8 bits per plane, lo rounded down, hi rounded
// up) and pack the 64-byte record (hr_types.h).  Shared by the collapse and by the refit.
HRD Node4 encodeNode4(const Box6 *cb, const Box6 &nb, int nValid, int nInner, uint32_t innerBase, int leafKey)
{
    uint32_t e[3];
    float inv[3];
    for (int k = 0; k < 3; ++k) {
        e[k] = quantExponent(nb.hi[k] - nb.lo[k]);
        inv[k] = 1.0f / __uint_as_float(e[k] << 23);
    }
    uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int c = 0; c < 4; ++c) {
        for (int k = 0; k < 3; ++k) {
            uint32_t lo8 = 255u, hi8 = 0u; // no child: inverted box (the traversal also checks the child count)
            if (c < nValid) {
                const float fl = floor_((cb[c].lo[k] - nb.lo[k]) * inv[k]);
                const float fh = __builtin_ceilf((cb[c].hi[k] - nb.lo[k]) * inv[k]);
                lo8 = (uint32_t)fmin_(fmax_(fl, 0.0f), 255.0f);
                hi8 = (uint32_t)fmin_(fmax_(fh, 0.0f), 255.0f);
            }
            qlo[k] |= lo8 << (8 * c);
            qhi[k] |= hi8 << (8 * c);
        }
    }
    Node4 nd;
    nd.a = make_float4(nb.lo[0], nb.lo[1], nb.lo[2],
                       __uint_as_float(e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)nInner << 24) | ((uint32_t)nValid << 27)));
    nd.b = make_uint4(qlo[0], qlo[1], qlo[2], qhi[0]);
    nd.c = make_uint4(qhi[1], qhi[2], innerBase, (uint32_t)leafKey);
    nd.d = make_uint4(0u, 0u, 0u, 0u);
    return nd;
}

// Collapse the binary tree into 4-wide nodes, one tree level per launch.  binOf[i] is the binary (Karras)
// node that 4-wide node i stands for.  Its (up to four) children are the descendants of that node which make the summed surface
// area of the 4-wide nodes below the least (the costs of k_refit_round).
// Leaves hold ONE triangle.  The inner children of a node are appended together through one atomic reservation
// (siblings become neighbours in memory), and so are its triangles, which are copied to their final place.
__global__ __launch_bounds__(256) void k_collapse4(const KNode *__restrict__ knodes, const Box6 *__restrict__ leafBox,
                                                   const Box6 *__restrict__ nodeBox, int *__restrict__ binOf, uint32_t levelStart,
                                                   uint32_t levelEnd, uint32_t *__restrict__ counter, uint32_t *__restrict__ leafCounter,
                                                   const Tri *__restrict__ sorted, Tri *__restrict__ finalTris, Node4 *__restrict__ out,
                                                   Box6 *__restrict__ nodeBoxOut, const SceneConsts *__restrict__ consts, const float4 *__restrict__ cost)
{
    const uint32_t i = levelStart + blockIdx.x * 256 + threadIdx.x;
    if (i >= levelEnd) return;
    const int b = binOf[i];
    int cand[4];
    // The children that minimise the summed area of the nodes below (k_refit_round's costs): binary node b is opened over four slots;
    // a child with a budget of k slots stays one child (a node of its own, or a triangle) unless opening it over those slots is cheaper.
    auto costOf = [&](int ref, int k) -> float {
        if (ref < 0) return 0.0f;
        const float4 c = cost[ref];
        return k == 1 ? c.x : (k == 2 ? c.y : (k == 3 ? c.z : c.w));
    };
    int stackRef[4], stackK[4], sp = 0, n = 0;
    stackRef[sp] = b, stackK[sp] = 4, ++sp;
    bool first = true;
    while (sp > 0) {
        --sp;
        const int ref = stackRef[sp], k = stackK[sp];
        const bool open = first || (ref >= 0 && k >= 2 && costOf(ref, k) < costOf(ref, 1));
        first = false;
        if (!open) {
            cand[n++] = ref;
            continue;
        }
        const int L = knodes[ref].left, R = knodes[ref].right;
        int bestL = 1;
        float best = costOf(L, 1) + costOf(R, k - 1);
        for (int jl = 2; jl < k; ++jl) {
            const float c = costOf(L, jl) + costOf(R, k - jl);
            if (c < best) best = c, bestL = jl;
        }
        stackRef[sp] = R, stackK[sp] = k - bestL, ++sp;
        stackRef[sp] = L, stackK[sp] = bestL, ++sp;
    }
    // inner children first, triangles after them (the order of the children inside a node is free)
    int ord[4];
    int nInner = 0;
    for (int c = 0; c < n; ++c)
        if (cand[c] >= 0) ord[nInner++] = cand[c];
    int nValid = nInner;
    for (int c = 0; c < n; ++c)
        if (cand[c] < 0) ord[nValid++] = cand[c];
    const int nLeaf = nValid - nInner;
    const uint32_t innerBase = nInner ? atomicAdd(counter, (uint32_t)nInner) : 0u;
    const uint32_t leafBase = nLeaf ? atomicAdd(leafCounter, (uint32_t)nLeaf) : 0u;
    Box6 cb[4];
    Box6 nb;
    for (int k = 0; k < 3; ++k) nb.lo[k] = __builtin_inff(), nb.hi[k] = -__builtin_inff();
    for (int c = 0; c < nValid; ++c) {
        const int ref = ord[c];
        if (ref < 0) {
            cb[c] = leafBox[~ref];
            finalTris[leafBase + (uint32_t)(nValid - 1 - c)] = sorted[~ref]; // descending with the child slot (see leafKey)
        } else {
            cb[c] = nodeBox[ref];
            binOf[innerBase + (uint32_t)c] = ref;
        }
        for (int k = 0; k < 3; ++k) nb.lo[k] = fmin_(nb.lo[k], cb[c].lo[k]), nb.hi[k] = fmax_(nb.hi[k], cb[c].hi[k]);
    }
    // child j >= nInner is triangle top - j with top = leafBase + nValid - 1: its reference ~(top - j) = ~top + j, so that a
    // child reference is `base + slot` for both kinds (base = innerBase or leafKey)
    const int leafKey = ~((int)leafBase + nValid - 1);
    out[i] = encodeNode4(cb, nb, nValid, nInner, innerBase, leafKey);
    nodeBoxOut[i] = nb;
}

// sum over the workgroup, then ONE float atomic (heuristic only: the order of the additions does not matter)
HRD void blockAreaAdd(float area, SceneConsts *consts, bool toTriangles = false)
{
    __shared__ float part[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = area;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = (part[0] + part[1]) + (part[2] + part[3]);
        if (t > 0.0f) atomicAdd(toTriangles ? &consts->triAreaSum : &consts->areaSum, t);
    }
}

// ---------------------------------------------------------------------------------------- refit
// One level of a bottom-up refit (levels are contiguous index ranges: nodes are allocated breadth-first).  A node's child
// boxes come from its triangles (leaf children; padded like at build time) and from the boxes its inner children wrote in
// the previous launch; its own box goes to nodeBox for the level above.  Same encoder as the build: conservative by construction.
__global__ __launch_bounds__(256) void k_refit4(Node4 *__restrict__ nodes, Box6 *__restrict__ nodeBox, const Tri *__restrict__ tris,
                                                uint32_t levelStart, uint32_t levelEnd, SceneConsts *__restrict__ consts)
{
    const uint32_t i = levelStart + blockIdx.x * 256 + threadIdx.x;
    float area = 0.0f;
    if (i < levelEnd) {
        const float pad = consts->pad;
        const Node4 nd = nodes[i];
        const uint32_t meta = __float_as_uint(nd.a.w);
        const int nInner = (int)((meta >> 24) & 7u), nValid = (int)(meta >> 27);
        const uint32_t innerBase = nd.c.z;
        const int leafKey = (int)nd.c.w;
        Box6 cb[4];
        Box6 nb;
        for (int k = 0; k < 3; ++k) nb.lo[k] = __builtin_inff(), nb.hi[k] = -__builtin_inff();
        for (int c = 0; c < nValid; ++c) {
            if (c < nInner) {
                cb[c] = nodeBox[innerBase + (uint32_t)c];
            } else {
                v3 bl, bh;
                triBounds(tris[~(leafKey + c)], bl, bh);
                cb[c].lo[0] = bl.x - pad, cb[c].lo[1] = bl.y - pad, cb[c].lo[2] = bl.z - pad;
                cb[c].hi[0] = bh.x + pad, cb[c].hi[1] = bh.y + pad, cb[c].hi[2] = bh.z + pad;
            }
            for (int k = 0; k < 3; ++k) nb.lo[k] = fmin_(nb.lo[k], cb[c].lo[k]), nb.hi[k] = fmax_(nb.hi[k], cb[c].hi[k]);
        }
        nodes[i] = encodeNode4(cb, nb, nValid, nInner, innerBase, leafKey);
        nodeBox[i] = nb;
        area = boxArea(nb);
    }
    blockAreaAdd(area, consts); // tree-quality heuristic: sum of node areas
}

// ---- the 32-byte nodes of k_trace (hr_types.h: Node32)
// biased exponent of the grid's cell along an axis of extent `ext`: the power of two with 256 cells > ext (so every frame origin is one of
// 256 grid points: a byte), kept inside the normal range with room for the scale exponents on both sides
HRD uint32_t gridCellExponent(float ext)
{
    const uint32_t e = (__float_as_uint(ext) >> 23) & 0xFFu; // ext < 2^(e - 126)
    const uint32_t c = e > 7u ? e - 7u : 0u;                  // 2^(c - 127) * 256 = 2^(e - 126) > ext
    return c < 24u ? 24u : (c > 230u ? 230u : c);
}
void gridOf(const SceneConsts &k, float gridLo[3], float gridCell[3], uint32_t gridCellExp[3])
{
    for (int a = 0; a < 3; ++a) {
        // (node boxes reach one leaf padding beyond the scene's bounds: the grid starts two paddings below them)
        gridLo[a] = k.lo[a] - 2.0f * k.pad;
        uint32_t bits;
        const float ext = (k.hi[a] + 2.0f * k.pad) - gridLo[a];
        std::memcpy(&bits, &ext, 4);
        const uint32_t e = (bits >> 23) & 0xFFu, c0 = e > 7u ? e - 7u : 0u, c = c0 < 24u ? 24u : (c0 > 230u ? 230u : c0);
        gridCellExp[a] = c;
        const uint32_t cb = c << 23;
        std::memcpy(&gridCell[a], &cb, 4);
    }
}
__global__ __launch_bounds__(256) void k_encode32(const Node4 *__restrict__ nodes, const Box6 *__restrict__ nodeBox, const Tri *__restrict__ tris, uint32_t nNodes,
                                                  const SceneConsts *__restrict__ consts, Node32 *__restrict__ out, int *__restrict__ leafKeys, SceneDev *__restrict__ scene)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float gLo[3], cell[3], invCell[3];
    uint32_t cexp[3];
    for (int k = 0; k < 3; ++k) {
        gLo[k] = consts->lo[k] - 2.0f * consts->pad; // (as gridOf on the host: same operations)
        cexp[k] = gridCellExponent((consts->hi[k] + 2.0f * consts->pad) - gLo[k]);
        cell[k] = __uint_as_float(cexp[k] << 23), invCell[k] = __uint_as_float((254u - cexp[k]) << 23);
    }
    if (i == 0 && scene)
        for (int k = 0; k < 3; ++k) scene->gridLo[k] = gLo[k], scene->gridCell[k] = cell[k], scene->gridCellExp[k] = cexp[k];
    if (i >= nNodes) return;
    const float pad = consts->pad;
    const Node4 nd = nodes[i];
    const uint32_t meta = __float_as_uint(nd.a.w);
    const int nInner = (int)((meta >> 24) & 7u), nValid = (int)(meta >> 27);
    const uint32_t innerBase = nd.c.z;
    const int leafKey = (int)nd.c.w;
    Box6 cb[4];
    Box6 nb;
    for (int k = 0; k < 3; ++k) nb.lo[k] = __builtin_inff(), nb.hi[k] = -__builtin_inff();
    for (int c = 0; c < nValid; ++c) {
        if (c < nInner) {
            cb[c] = nodeBox[innerBase + (uint32_t)c];
        } else {
            v3 bl, bh;
            triBounds(tris[~(leafKey + c)], bl, bh);
            cb[c].lo[0] = bl.x - pad, cb[c].lo[1] = bl.y - pad, cb[c].lo[2] = bl.z - pad;
            cb[c].hi[0] = bh.x + pad, cb[c].hi[1] = bh.y + pad, cb[c].hi[2] = bh.z + pad;
        }
        for (int k = 0; k < 3; ++k) nb.lo[k] = fmin_(nb.lo[k], cb[c].lo[k]), nb.hi[k] = fmax_(nb.hi[k], cb[c].hi[k]);
    }
    // frame: the grid point at or below the node's lower corner and, per axis, the smallest
    // power-of-two number of cells from there that holds the node: hi <= origin + 255 * scale with scale = cell * 2^(e - 8)
    // The origin is taken in float64, where gLo + g * cell is EXACT: that sum is what the traversal's decode stands for (rayFrame32 folds
    // gLo and cell into the ray's constants separately), and as a float32 it is rounded by up to half an ulp of the coordinate once the
    // scene lies 2^10 or so extents from the world's origin — more than the leaf padding there, so planes quantised against the rounded
    // origin cut into triangles (tests/tree_audit.py found it: -3.4 hit_pad on the soup at 2^10).  The differences below are exact in
    // float64 too (two float32 values whose exponents lie within 29 of each other), so floor and ceil see true quotients.
    uint32_t g[3], e[3];
    double origin[3];
    for (int k = 0; k < 3; ++k) {
        const float f = floor_((nb.lo[k] - gLo[k]) * invCell[k]);
        g[k] = (uint32_t)fmin_(fmax_(f, 0.0f), 255.0f);
        origin[k] = (double)gLo[k] + (double)g[k] * (double)cell[k];
        if (origin[k] > (double)nb.lo[k] && g[k] > 0u) g[k] -= 1u, origin[k] = (double)gLo[k] + (double)g[k] * (double)cell[k]; // (the rounding of f)
        e[k] = 0u;
        while (e[k] < 15u && (double)nb.hi[k] - origin[k] > 255.0 * (double)__uint_as_float((cexp[k] + e[k] - 8u) << 23)) ++e[k];
    }
    uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        const double inv = (double)__uint_as_float((254u - (cexp[k] + e[k] - 8u)) << 23); // 1 / scale
        for (int c = 0; c < 4; ++c) {
            uint32_t lo8 = 255u, hi8 = 0u; // no child: inverted planes, never entered
            if (c < nValid) {
                const double fl = __builtin_floor(((double)cb[c].lo[k] - origin[k]) * inv);
                const double fh = __builtin_ceil(((double)cb[c].hi[k] - origin[k]) * inv);
                lo8 = (uint32_t)(fl < 0.0 ? 0.0 : (fl > 255.0 ? 255.0 : fl));
                hi8 = (uint32_t)(fh < 0.0 ? 0.0 : (fh > 255.0 ? 255.0 : fh));
            }
            qlo[k] |= lo8 << (8 * c);
            qhi[k] |= hi8 << (8 * c);
        }
    }
    Node32 o;
    o.p = make_uint4(qlo[0], qlo[1], qlo[2], qhi[0]);
    o.q = make_uint4(qhi[1], qhi[2], (innerBase & 0x01FFFFFFu) | ((uint32_t)nInner << 25) | (e[0] << 28), g[0] | (g[1] << 8) | (g[2] << 16) | (e[1] << 24) | (e[2] << 28));
    out[i] = o;
    leafKeys[i] = leafKey; // (the one word of Node4 k_trace still needs: a compact array that stays in L2)
}
void encodeNodes32(hipStream_t st, const BuildResult &tree, const SceneConsts *consts, SceneDev *scene)
{
    const uint32_t n = tree.nNodes > 0 ? (uint32_t)tree.nNodes : 0u;
    if (!tree.nodes32 && n) return;
    hipLaunchKernelGGL(k_encode32, dim3(n ? (n + 255) / 256 : 1), dim3(256), 0, st, tree.nodes, tree.nodeBox, tree.tris, n, consts, tree.nodes32, tree.leafKeys, scene);
}

void refitLBVH(hipStream_t st, const BuildResult &tree, uint32_t nTris, SceneConsts *consts)
{
    (void)nTris;
    for (int level = tree.levels - 1; level >= 0; --level) {
        const uint32_t a = tree.levelStart[level], b = tree.levelStart[level + 1];
        if (b > a) hipLaunchKernelGGL(k_refit4, dim3((b - a + 255) / 256), dim3(256), 0, st, tree.nodes, tree.nodeBox, tree.tris, a, b, consts);
    }
}

__global__ __launch_bounds__(256) void k_slot_of_prim(const Tri *__restrict__ leafTris, uint32_t n, uint32_t *__restrict__ slotOfPrim)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = __float_as_uint(leafTris[i].r.y);
    if (prim != 0xFFFFFFFFu) slotOfPrim[prim] = i; // (a slot a cached tree left unused carries prim id ~0)
}

__global__ __launch_bounds__(256) void k_area_sum(const Box6 *__restrict__ nodeBox, uint32_t n, SceneConsts *__restrict__ consts)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    blockAreaAdd(i < n ? boxArea(nodeBox[i]) : 0.0f, consts);
}
void launchAreaSum(hipStream_t st, const Box6 *nodeBox, uint32_t n, SceneConsts *consts)
{
    if (n) hipLaunchKernelGGL(k_area_sum, dim3((n + 255) / 256), dim3(256), 0, st, nodeBox, n, consts);
}
// sum of the triangles' own areas, 0.5 |e1 x e2| (leaf-order array; unused slots of the 32-byte node formats carry prim id ~0)
__global__ __launch_bounds__(256) void k_tri_area_sum(const Tri *__restrict__ leafTris, uint32_t n, SceneConsts *__restrict__ consts)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float area = 0.0f;
    if (i < n) {
        const float4 p = leafTris[i].p, q = leafTris[i].q, r = leafTris[i].r;
        if (__float_as_uint(r.y) != 0xFFFFFFFFu) {
            const v3 e1(p.w, q.x, q.y), e2(q.z, q.w, r.x);
            const float a = 0.5f * length(cross(e1, e2));
            area = (a == a && a < 3.0e38f) ? a : 0.0f;
        }
    }
    blockAreaAdd(area, consts, true);
}
void launchTriAreaSum(hipStream_t st, const Tri *leafTris, uint32_t nSlots, SceneConsts *consts)
{
    if (nSlots) hipLaunchKernelGGL(k_tri_area_sum, dim3((nSlots + 255) / 256), dim3(256), 0, st, leafTris, nSlots, consts);
}

// ------------------------------------------------------------------------------- SAH subtrees
// The radix tree splits by Morton prefix, blind to the boxes.  Its bottom subtrees (at most T <= 64 triangles under a node of more) are
// rebuilt top-down by full-sweep SAH, one wave per subtree with a triangle per lane (hr_sah_subtree.h has the arithmetic and the CPU
// test), into the node slots the radix subtree owned.  The leaves keep their names (~sorted index): leafBox, the sorted triangles and
// with them PLOC's input stay as they are.  The rebuild runs AFTER the first bottom-up refit: a subtree's collapse cost C1 and its
// height (its stamp) are then known, the scene's cost before the rebuild can be reported, and the sweep's version is kept only where
// its C1 is lower and it is not deeper — the scene's cost never rises and the radix tree's 58-level bound holds.  The nodes above the
// subtrees are then refitted once more (k_sah_find clears their stamps).  tools/tree_proto.py: -5.1 % summed node area on the soup.
struct SahWork {
    int child, parent, side; // the subtree's root, the node above it, 0 / 1: it is the parent's left / right child
};

// one thread per radix node of more than T triangles: its stamp is cleared, its inner children of 3..T triangles are work items
__global__ __launch_bounds__(256) void k_sah_find(const KNode *__restrict__ nodes, int nInternal, int T, uint32_t *__restrict__ stamp,
                                                  SahWork *__restrict__ work, uint32_t maxWork, uint32_t *__restrict__ counters)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nInternal) return;
    const KNode k = nodes[i];
    if (k.last - k.first + 1 <= T) return;
    stamp[i] = 0u;
    for (int side = 0; side < 2; ++side) {
        const int ch = side ? k.right : k.left;
        if (ch < 0) continue;
        const int m = nodes[ch].last - nodes[ch].first + 1;
        if (m > T || m < 3) continue;
        const uint32_t at = atomicAdd(counters, 1u);
        if (at < maxWork) work[at] = SahWork{ch, i, side}; // (always: the items' triangles are disjoint and each has three)
    }
}

__global__ __launch_bounds__(64) void k_sah_subtrees(KNode *__restrict__ nodes, const Box6 *__restrict__ leafBox, Box6 *__restrict__ nodeBox,
                                                     float4 *__restrict__ cost, uint32_t *__restrict__ stamp, const SahWork *__restrict__ work,
                                                     uint32_t *__restrict__ counters)
{
    __shared__ SahSub s;
    const SahWork item = work[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int first = nodes[item.child].first, last = nodes[item.child].last;
    const int m = last - first + 1; // 3 .. 64 (k_sah_find)
    const int radixDepth = (int)stamp[item.child]; // (the round of the refit that finished it = its height)
    const float radixC1 = cost[item.child].x;
    if (lane == 0) s.m = m;
    if (lane < m) {
        const Box6 b = leafBox[first + lane];
        for (int q = 0; q < 3; ++q) s.lo[q][lane] = b.lo[q], s.hi[q][lane] = b.hi[q];
    }
    __syncthreads();
    sahInit(s, lane);
    __syncthreads();
    int levels = 0;
    for (;;) {
        sahCandidate(s, lane, levels & 1);
        __syncthreads();
        const bool more = sahPartition(s, lane, levels & 1, levels);
        ++levels;
        if (!__syncthreads_or(more ? 1 : 0)) break;
        if (levels >= radixDepth) return; // deeper than the radix subtree: that one stays (uniform: both values are the wave's)
    }
    for (int lv = levels - 1; lv >= 0; --lv) {
        sahEvaluate(s, lane, lv);
        __syncthreads();
    }
    if (!sahKeep(s.cost[0].c1, levels, radixC1, radixDepth)) return;
    const int base = sahOwnedBase(first, last, item.child);
    if (lane < m - 1) {
        const int l = s.left[lane], r = s.right[lane];
        KNode k;
        k.left = l < 0 ? ~(first + ~l) : base + l, k.right = r < 0 ? ~(first + ~r) : base + r;
        k.first = 0, k.last = 0; // (as PLOC's nodes: nothing reads a range after k_sah_find)
        Box6 b;
        for (int q = 0; q < 3; ++q) b.lo[q] = s.nlo[q][lane], b.hi[q] = s.nhi[q][lane];
        const SahCost c = s.cost[lane];
        nodes[base + lane] = k;
        nodeBox[base + lane] = b;
        cost[base + lane] = make_float4(c.c1, c.c2, c.c3, c.c4);
        stamp[base + lane] = 1u; // finished before every round of the refit that follows
    }
    if (lane == 0) {
        if (base != item.child) { // the root moved to the first owned slot: the parent's link follows
            if (item.side)
                nodes[item.parent].right = base;
            else
                nodes[item.parent].left = base;
        }
        atomicAdd(counters + 1, 1u);
    }
}

// ------------------------------------------------------------------------------------------- PLOC
// Parallel locally-ordered clustering (Meister & Bittner 2018) over the Morton-ordered triangle boxes: in every iteration each cluster
// looks for its nearest neighbour (smallest surface area of the merged box) among the r clusters before and behind it in the array,
// mutual nearest neighbours merge, the array is compacted.  The binary tree that results is what the radix tree of k_karras is for the
// LBVH: input of the same DP collapse to 4-wide nodes.  On meshes it is the better tree (terrain: -17 % summed node area, i.e. node
// visits per ray; tools/tree_proto.py, profiles/r4_tree_proto.txt); on the benchmark's uniform triangle fog spatial-median splits are
// within 7 % of a full-sweep SAH build and PLOC is 2-6 % WORSE than the LBVH — so buildLBVH builds both and keeps the cheaper one.
#ifndef HR_PLOC_RADIUS_MAX
#define HR_PLOC_RADIUS_MAX 32
#endif
HRD float unionArea(const Box6 &a, const Box6 &b)
{
    const float dx = fmax_(a.hi[0], b.hi[0]) - fmin_(a.lo[0], b.lo[0]), dy = fmax_(a.hi[1], b.hi[1]) - fmin_(a.lo[1], b.lo[1]),
                dz = fmax_(a.hi[2], b.hi[2]) - fmin_(a.lo[2], b.lo[2]);
    return dx * dy + dy * dz + dz * dx;
}

// state of the clustering on the device: [0] clusters in the array, [1] binary nodes made so far
__global__ __launch_bounds__(256) void k_ploc_nn(const Box6 *__restrict__ box, const uint32_t *__restrict__ state, int r, uint32_t *__restrict__ nn)
{
    __shared__ Box6 tile[256 + 2 * HR_PLOC_RADIUS_MAX];
    const int m = (int)state[0];
    const int base = (int)blockIdx.x * 256;
    if (base >= m) return;
    for (int t = threadIdx.x; t < 256 + 2 * r; t += 256) {
        const int g = base - r + t;
        if (g >= 0 && g < m) tile[t] = box[g];
    }
    __syncthreads();
    const int i = base + (int)threadIdx.x;
    if (i >= m) return;
    const Box6 me = tile[threadIdx.x + r];
    // the candidate with the smallest key (area, |i - j|, parity of min(i, j), min(i, j)) — a key that is the same seen from both ends
    // of a pair, so the pair with the globally smallest key is always mutual and every iteration merges at least one pair; among equal
    // areas (coincident or regularly spaced triangles) the nearest index wins and then the pair (2k, 2k + 1), so that a run of equal
    // boxes pairs up completely in one iteration instead of one pair at a time
    float best = __builtin_inff();
    int bestJ = -1;
    for (int off = -r; off <= r; ++off) {
        const int j = i + off;
        if (off == 0 || j < 0 || j >= m) continue;
        const float a = unionArea(me, tile[(int)threadIdx.x + r + off]);
        bool better = bestJ < 0 || a < best;
        if (!better && a == best) {
            const int d1 = off < 0 ? -off : off, d0 = bestJ > i ? bestJ - i : i - bestJ;
            const int lo1 = i < j ? i : j, lo0 = i < bestJ ? i : bestJ;
            better = d1 < d0 || (d1 == d0 && ((lo1 & 1) < (lo0 & 1) || ((lo1 & 1) == (lo0 & 1) && lo1 < lo0)));
        }
        if (better) best = a, bestJ = j;
    }
    nn[i] = (uint32_t)bestJ;
}

// PHASE 0: per workgroup, how many clusters stay in the array and how many pairs merge (packed: stay | merge << 32).
// PHASE 1: with those counts turned into exclusive prefixes, write the next array: a merging pair becomes a new binary node (its box,
// its collapse costs: both children exist since an earlier launch) at the place of its lower member; the higher member disappears.
template <int PHASE>
__global__ __launch_bounds__(256) void k_ploc_merge(const uint32_t *__restrict__ state, const uint32_t *__restrict__ nn, const int *__restrict__ refIn,
                                                    const Box6 *__restrict__ boxIn, unsigned long long *__restrict__ blockSums, int *__restrict__ refOut,
                                                    Box6 *__restrict__ boxOut, KNode *__restrict__ knodes, Box6 *__restrict__ nodeBox, float4 *__restrict__ cost)
{
    __shared__ uint32_t wk[4], wm[4];
    const uint32_t m = state[0];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= m) return; // (uniform)
    bool keep = false, makes = false;
    uint32_t j = 0;
    if (i < m) {
        j = nn[i];
        const bool mutual = j < m && nn[j] == i;
        keep = !(mutual && j < i);
        makes = mutual && i < j;
    }
    const unsigned long long kb = __ballot(keep), mb = __ballot(makes);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wk[wave] = (uint32_t)__popcll(kb), wm[wave] = (uint32_t)__popcll(mb);
    __syncthreads();
    if (PHASE == 0) {
        if (threadIdx.x == 0) blockSums[blockIdx.x] = (unsigned long long)(wk[0] + wk[1] + wk[2] + wk[3]) | ((unsigned long long)(wm[0] + wm[1] + wm[2] + wm[3]) << 32);
        return;
    }
    uint32_t kBefore = 0, mBefore = 0;
    for (uint32_t w = 0; w < wave; ++w) kBefore += wk[w], mBefore += wm[w];
    const unsigned long long pre = blockSums[blockIdx.x], lt = (1ull << lane) - 1ull;
    const uint32_t pos = (uint32_t)pre + kBefore + (uint32_t)__popcll(kb & lt);
    if (makes) {
        const uint32_t id = state[1] + (uint32_t)(pre >> 32) + mBefore + (uint32_t)__popcll(mb & lt);
        const Box6 a = boxIn[i], b = boxIn[j];
        Box6 u;
#pragma unroll
        for (int c = 0; c < 3; ++c) u.lo[c] = fmin_(a.lo[c], b.lo[c]), u.hi[c] = fmax_(a.hi[c], b.hi[c]);
        KNode k;
        k.left = refIn[i], k.right = refIn[j], k.first = 0, k.last = 0;
        knodes[id] = k;
        nodeBox[id] = u;
        cost[id] = collapseCost(k.left, k.right, boxArea(u), cost);
        refOut[pos] = (int)id;
        boxOut[pos] = u;
    } else if (keep) {
        refOut[pos] = refIn[i];
        boxOut[pos] = boxIn[i];
    }
}

// exclusive scan of n packed (low | high << 32) counters by ONE workgroup; then the iteration's totals update the state
__global__ __launch_bounds__(1024) void k_ploc_scan(unsigned long long *__restrict__ data, uint32_t *__restrict__ state)
{
    __shared__ unsigned long long waveSums[16];
    __shared__ unsigned long long carry;
    const uint32_t n = (state[0] + 255u) / 256u;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = (i < n) ? data[i] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(inc, o);
            if ((int)lane >= o) inc += t;
        }
        if (lane == 63) waveSums[wave] = inc;
        __syncthreads();
        unsigned long long wavePrefix = 0;
        for (uint32_t w = 0; w < wave; ++w) wavePrefix += waveSums[w];
        const unsigned long long c = carry;
        if (i < n) data[i] = c + wavePrefix + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + wavePrefix + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        state[2] = (uint32_t)carry;         // clusters of the next array
        state[3] = (uint32_t)(carry >> 32); // nodes made by this iteration
    }
}
__global__ void k_ploc_advance(uint32_t *state)
{
    state[0] = state[2];
    state[1] += state[3];
}
__global__ __launch_bounds__(256) void k_ploc_init(const Box6 *__restrict__ leafBox, uint32_t n, int *__restrict__ ref, Box6 *__restrict__ box)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ref[i] = ~(int)i;
    box[i] = leafBox[i];
}

// The last iterations in ONE workgroup: once at most kPlocTail clusters are left they live in LDS and the remaining ~20 iterations (each
// of which was five launches and a 4-byte read-back) run without leaving the kernel.  Same nearest-neighbour rule, same pair rule, same
// order of the new nodes (array order) as the iterations above, so the tree does not depend on where the hand-over happens.
static const int kPlocTail = 1024;
__global__ __launch_bounds__(kPlocTail) void k_ploc_tail(uint32_t *__restrict__ state, const int *__restrict__ refIn, const Box6 *__restrict__ boxIn, int r,
                                                        KNode *__restrict__ knodes, Box6 *__restrict__ nodeBox, float4 *cost /* read back inside the launch: no restrict */)
{
    __shared__ Box6 sbox[2][kPlocTail];
    __shared__ int sref[2][kPlocTail];
    __shared__ int snn[kPlocTail];
    __shared__ uint32_t wk[kPlocTail / 64], wm[kPlocTail / 64];
    const int t = (int)threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int m = (int)state[0];
    uint32_t base = state[1];
    if (t < m) sbox[0][t] = boxIn[t], sref[0][t] = refIn[t];
    __syncthreads();
    int cur = 0;
    while (m > 1) {
        // nearest neighbour (k_ploc_nn's rule)
        int bestJ = -1;
        if (t < m) {
            const Box6 me = sbox[cur][t];
            float best = __builtin_inff();
            for (int off = -r; off <= r; ++off) {
                const int j = t + off;
                if (off == 0 || j < 0 || j >= m) continue;
                const float a = unionArea(me, sbox[cur][j]);
                bool better = bestJ < 0 || a < best;
                if (!better && a == best) {
                    const int d1 = off < 0 ? -off : off, d0 = bestJ > t ? bestJ - t : t - bestJ;
                    const int lo1 = t < j ? t : j, lo0 = t < bestJ ? t : bestJ;
                    better = d1 < d0 || (d1 == d0 && ((lo1 & 1) < (lo0 & 1) || ((lo1 & 1) == (lo0 & 1) && lo1 < lo0)));
                }
                if (better) best = a, bestJ = j;
            }
            snn[t] = bestJ;
        }
        __syncthreads();
        bool keep = false, makes = false;
        int j = 0;
        if (t < m) {
            j = snn[t];
            const bool mutual = j >= 0 && j < m && snn[j] == t;
            keep = !(mutual && j < t);
            makes = mutual && t < j;
        }
        const unsigned long long kb = __ballot(keep), mb = __ballot(makes);
        if (lane == 0) wk[wave] = (uint32_t)__popcll(kb), wm[wave] = (uint32_t)__popcll(mb);
        __syncthreads();
        uint32_t kBefore = 0, mBefore = 0, kTotal = 0, mTotal = 0;
        for (uint32_t w = 0; w < (uint32_t)(kPlocTail / 64); ++w) {
            kBefore += w < wave ? wk[w] : 0u, mBefore += w < wave ? wm[w] : 0u;
            kTotal += wk[w], mTotal += wm[w];
        }
        const unsigned long long lt = (1ull << lane) - 1ull;
        const uint32_t pos = kBefore + (uint32_t)__popcll(kb & lt);
        if (makes) {
            const uint32_t id = base + mBefore + (uint32_t)__popcll(mb & lt);
            const Box6 a = sbox[cur][t], b = sbox[cur][j];
            Box6 u;
#pragma unroll
            for (int c = 0; c < 3; ++c) u.lo[c] = fmin_(a.lo[c], b.lo[c]), u.hi[c] = fmax_(a.hi[c], b.hi[c]);
            KNode k;
            k.left = sref[cur][t], k.right = sref[cur][j], k.first = 0, k.last = 0;
            knodes[id] = k;
            nodeBox[id] = u;
            // (a child made earlier in THIS launch was written by another thread: visible after the barrier below and the fence)
            cost[id] = collapseCost(k.left, k.right, boxArea(u), cost);
            sref[cur ^ 1][pos] = (int)id;
            sbox[cur ^ 1][pos] = u;
        } else if (keep) {
            sref[cur ^ 1][pos] = sref[cur][t];
            sbox[cur ^ 1][pos] = sbox[cur][t];
        }
        __threadfence();
        __syncthreads();
        m = (int)kTotal, base += mTotal, cur ^= 1;
        // An iteration that merged nothing would repeat itself for ever, one workgroup spinning until the GPU is reset.  The pair key
        // reads the same from both ends, so it cannot happen for ordered areas — but NaN boxes (non-finite vertices) are not ordered.
        // mTotal comes from LDS totals every thread has read alike: a uniform exit; state[1] != n - 1 then tells buildPLOC (rc 7:
        // the radix tree is kept).
        if (mTotal == 0u) break;
    }
    if (t == 0) state[0] = (uint32_t)m, state[1] = base;
}

// ------------------------------------------------------------------------------ the build on the host
namespace {
// Device scratch of a build: every array it hands out is freed when the holder goes out of scope, on whichever path its function is left.
struct Scratch {
    std::vector<void *> held;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    ~Scratch() { for (void *p : held) hipFree(p); }
    template <class T> bool alloc(T *&p, size_t count)
    {
        if (hipMalloc(&p, sizeof(T) * count) != hipSuccess) return false;
        held.push_back(p);
        return true;
    }
    // the array stops being scratch: it is the caller's from here on
    template <class T> T *release(T *p)
    {
        held.erase(std::remove(held.begin(), held.end(), (void *)p), held.end());
        return p;
    }
};

// What the stages of buildLBVH hand to one another.  A stage returns 0 or the build's return code; `mem` frees everything on every path.
struct Build {
    hipStream_t st;
    uint32_t n; // triangles
    const BuildOptions &opt;
    BuildResult *out;
    Scratch mem;
    uint32_t *keys = nullptr;                     // sortByMorton: the sorted keys,
    Tri *sorted = nullptr, *finalTris = nullptr;  // the triangles in their order (collapse: in leaf order)
    Box6 *leafBox = nullptr;                      // and their padded boxes
    int nInternal = 0;                            // radixTree: n - 1 binary nodes, the root is node 0
    uint32_t gi = 0;                              // workgroups of a launch over them
    KNode *knodes = nullptr, *pKnodes = nullptr;  // the radix tree (sahSubtrees rewrites parts of it) and plocCandidate's tree: nodes,
    Box6 *nodeBox = nullptr, *pBox = nullptr;     // boxes
    float4 *cost = nullptr, *pCost = nullptr;     // and costs of the collapse (k_refit_round, k_collapse4)
    uint32_t *stamp = nullptr, rootStamp = 0;     // the round that finished each radix node; the root's = the tree's height
    int pRoot = 0;                                // the PLOC tree's root
    bool usePloc = false;                         // ... and whether it is the tree to collapse
};
} // namespace

// Refit rounds (k_refit_round) numbered from `first` until the root is stamped, `limit` rounds at the most; the host looks at the root's
// stamp after every 16th round counted from the first.  b.rootStamp = what it saw last (0: the root was not finished at that look).
static int refitToRoot(Build &b, uint32_t first, uint32_t limit)
{
    b.rootStamp = 0;
    for (uint32_t k = 1; k <= limit && b.rootStamp == 0; ++k) {
        hipLaunchKernelGGL(k_refit_round, dim3(b.gi), dim3(256), 0, b.st, b.knodes, b.nInternal, b.leafBox, b.nodeBox, b.stamp, first + k - 1u, b.cost);
        if ((k & 15u) == 0u) {
            HR_CHECK(hipMemcpyAsync(&b.rootStamp, b.stamp, 4, hipMemcpyDeviceToHost, b.st));
            HR_CHECK(hipStreamSynchronize(b.st));
        }
    }
    return 0;
}

// a tree's collapse cost C1 over the surface area of the root's box (0 for a flat root): what BuildResult reports
static float costOverRootArea(const float4 &c, const Box6 &root)
{
    const float dx = root.hi[0] - root.lo[0], dy = root.hi[1] - root.lo[1], dz = root.hi[2] - root.lo[2];
    const float ra = dx * dy + dy * dz + dz * dx;
    return ra > 0.0f ? c.x / ra : 0.0f;
}

static int sortByMorton(Build &b, const Tri *trisPrim, const float lo[3], const float hi[3], float pad)
{
    const uint32_t n = b.n, nBlocks = (n + kSortTile - 1) / kSortTile, g256 = (n + 255) / 256;
    uint32_t *keysA, *keysB, *valsA, *valsB, *blockHist;
    if (!(b.mem.alloc(keysA, n) && b.mem.alloc(keysB, n) && b.mem.alloc(valsA, n) && b.mem.alloc(valsB, n) && b.mem.alloc(blockHist, 256ull * nBlocks) &&
          b.mem.alloc(b.sorted, n) && b.mem.alloc(b.leafBox, n)))
        return 1;
    const v3 vlo(lo[0], lo[1], lo[2]);
    const v3 ext(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
    hipLaunchKernelGGL(k_morton, dim3(g256), dim3(256), 0, b.st, trisPrim, n, vlo, ext, keysA, valsA);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass * 8;
        hipLaunchKernelGGL(k_sort_hist, dim3(nBlocks), dim3(64), 0, b.st, keysA, n, shift, blockHist, nBlocks);
        hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, b.st, blockHist, 256u * nBlocks, (uint32_t *)nullptr);
        hipLaunchKernelGGL(k_sort_scatter, dim3(nBlocks), dim3(64), 0, b.st, keysA, valsA, n, shift, blockHist, nBlocks, keysB, valsB);
        std::swap(keysA, keysB);
        std::swap(valsA, valsB);
    }
    hipLaunchKernelGGL(k_gather_tris, dim3(g256), dim3(256), 0, b.st, trisPrim, valsA, n, b.sorted, pad, b.leafBox);
    b.keys = keysA;
    return 0;
}

// the radix tree over the sorted keys, with its boxes and collapse costs
static int radixTree(Build &b)
{
    b.nInternal = (int)b.n - 1;
    b.gi = (uint32_t)(b.nInternal + 255) / 256;
    if (!(b.mem.alloc(b.knodes, b.nInternal) && b.mem.alloc(b.nodeBox, b.nInternal) && b.mem.alloc(b.stamp, b.nInternal) && b.mem.alloc(b.cost, b.nInternal)))
        return 1;
    HR_CHECK(hipMemsetAsync(b.stamp, 0, 4ull * b.nInternal, b.st));
    hipLaunchKernelGGL(k_karras, dim3(b.gi), dim3(256), 0, b.st, b.keys, (int)b.n, b.knodes);
    // tree height <= 30 key bits + 28 index bits
    if (int rc = refitToRoot(b, 1u, 64u)) return rc;
    return b.rootStamp == 0 ? 3 : 0; // (the last of the 64 rounds is one the host looks after)
}

// the radix tree's bottom subtrees rebuilt by full-sweep SAH (k_sah_subtrees), then the nodes above them refitted again
static int sahSubtrees(Build &b)
{
    const int sahT = b.opt.sahSub > kSahMax ? kSahMax : b.opt.sahSub;
    if (sahT < 3 || b.n <= (uint32_t)sahT) return 0;
    const uint32_t maxWork = b.n / 3u + 1u;
    Scratch mem;
    SahWork *work;
    uint32_t *counters; // [0] subtrees found, [1] replaced
    float4 c0{}, c1{};
    Box6 rootBox{};
    uint32_t found[2] = {0u, 0u};
    if (!(mem.alloc(work, maxWork) && mem.alloc(counters, 2))) return 1;
    HR_CHECK(hipMemsetAsync(counters, 0, 8, b.st));
    hipLaunchKernelGGL(k_sah_find, dim3(b.gi), dim3(256), 0, b.st, b.knodes, b.nInternal, sahT, b.stamp, work, maxWork, counters);
    HR_CHECK(hipMemcpyAsync(found, counters, 4, hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipMemcpyAsync(&c0, b.cost, sizeof(float4), hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipMemcpyAsync(&rootBox, b.nodeBox, sizeof(Box6), hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipStreamSynchronize(b.st));
    if (found[0] > maxWork) return 8; // (cannot happen: see k_sah_find)
    if (found[0] > 0u) hipLaunchKernelGGL(k_sah_subtrees, dim3(found[0]), dim3(64), 0, b.st, b.knodes, b.leafBox, b.nodeBox, b.cost, b.stamp, work, counters);
    // (k_sah_find has cleared the stamps of the nodes above: the old stamps below them are <= rootStamp, the new ones 1)
    if (int rc = refitToRoot(b, b.rootStamp + 1u, 64u)) return rc;
    HR_CHECK(hipMemcpyAsync(&b.rootStamp, b.stamp, 4, hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipMemcpyAsync(found + 1, counters + 1, 4, hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipMemcpyAsync(&c1, b.cost, sizeof(float4), hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipStreamSynchronize(b.st));
    if (b.rootStamp == 0) return 3;
    b.out->sahCostBefore = costOverRootArea(c0, rootBox), b.out->sahCostAfter = costOverRootArea(c1, rootBox);
    b.out->sahFound = found[0], b.out->sahReplaced = found[1];
    return 0;
}

// Binary tree over the sorted triangles by PLOC: knodes / nodeBox / cost have n - 1 entries; *rootOut is the root's index (n - 2).
// Returns 0, or non-zero when it did not finish (the caller then keeps the radix tree).
static int buildPLOC(hipStream_t st, const Box6 *leafBox, uint32_t n, int radius, KNode *knodes, Box6 *nodeBox, float4 *cost, int *rootOut)
{
    Scratch mem;
    int *ref[2];
    Box6 *box[2];
    uint32_t *nn, *state;
    unsigned long long *sums;
    const uint32_t nb0 = (n + 255) / 256;
    if (!(mem.alloc(ref[0], n) && mem.alloc(ref[1], n) && mem.alloc(box[0], n) && mem.alloc(box[1], n) && mem.alloc(nn, n) && mem.alloc(state, 4) &&
          mem.alloc(sums, nb0)))
        return 1;
    const uint32_t init[4] = {n, 0u, 0u, 0u};
    HR_CHECK(hipMemcpyAsync(state, init, 16, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ploc_init, dim3(nb0), dim3(256), 0, st, leafBox, n, ref[0], box[0]);
    const int r = radius < 1 ? 1 : (radius > HR_PLOC_RADIUS_MAX ? HR_PLOC_RADIUS_MAX : radius);
    uint32_t m = n;
    int cur = 0;
    // every iteration merges at least one pair (k_ploc_nn), typically a third of the clusters: ~45 iterations for a million
    // triangles.  The host reads the cluster count back after each (a 4-byte copy: the launches are sized by it).
    for (uint32_t it = 0; m > (uint32_t)kPlocTail; ++it) {
        if (it >= 4096u) return 7; // (a pathological input that merges a pair at a time: not worth it, the radix tree is kept)
        const uint32_t nb = (m + 255) / 256;
        hipLaunchKernelGGL(k_ploc_nn, dim3(nb), dim3(256), 0, st, box[cur], state, r, nn);
        hipLaunchKernelGGL((k_ploc_merge<0>), dim3(nb), dim3(256), 0, st, state, nn, ref[cur], box[cur], sums, ref[cur ^ 1], box[cur ^ 1], knodes, nodeBox, cost);
        hipLaunchKernelGGL(k_ploc_scan, dim3(1), dim3(1024), 0, st, sums, state);
        hipLaunchKernelGGL((k_ploc_merge<1>), dim3(nb), dim3(256), 0, st, state, nn, ref[cur], box[cur], sums, ref[cur ^ 1], box[cur ^ 1], knodes, nodeBox, cost);
        hipLaunchKernelGGL(k_ploc_advance, dim3(1), dim3(1), 0, st, state);
        uint32_t mNew = 0;
        HR_CHECK(hipMemcpyAsync(&mNew, state, 4, hipMemcpyDeviceToHost, st));
        HR_CHECK(hipStreamSynchronize(st));
        if (mNew >= m || mNew == 0) return 7; // (cannot happen: see k_ploc_nn)
        m = mNew;
        cur ^= 1;
    }
    if (m > 1) hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(kPlocTail), 0, st, state, ref[cur], box[cur], r, knodes, nodeBox, cost);
    uint32_t made = 0;
    HR_CHECK(hipMemcpyAsync(&made, state + 1, 4, hipMemcpyDeviceToHost, st));
    HR_CHECK(hipStreamSynchronize(st));
    *rootOut = (int)n - 2;
    return made == n - 1 ? 0 : 7;
}

// The second candidate: the PLOC tree over the same sorted triangles; the one whose collapse costs less (summed surface area of the
// 4-wide nodes = expected node visits of a random ray) is kept.  A PLOC tree that could not be built is no error: the radix tree stays.
static int plocCandidate(Build &b)
{
    if (b.opt.ploc == 0 || b.n < 4u) return 0;
    bool ok = b.mem.alloc(b.pKnodes, b.nInternal) && b.mem.alloc(b.pBox, b.nInternal) && b.mem.alloc(b.pCost, b.nInternal) &&
              buildPLOC(b.st, b.leafBox, b.n, b.opt.plocRadius, b.pKnodes, b.pBox, b.pCost, &b.pRoot) == 0;
    float4 cR{}, cP{};
    Box6 rootBox{};
    ok = ok && hipMemcpyAsync(&cR, b.cost, sizeof(float4), hipMemcpyDeviceToHost, b.st) == hipSuccess &&
         hipMemcpyAsync(&cP, b.pCost + b.pRoot, sizeof(float4), hipMemcpyDeviceToHost, b.st) == hipSuccess &&
         hipMemcpyAsync(&rootBox, b.nodeBox, sizeof(Box6), hipMemcpyDeviceToHost, b.st) == hipSuccess && hipStreamSynchronize(b.st) == hipSuccess;
    if (ok) {
        b.out->costRadix = costOverRootArea(cR, rootBox), b.out->costPloc = costOverRootArea(cP, rootBox);
        // PLOC has to win clearly (5 %): the surface-area measure assumes rays distributed like random lines through the root box,
        // while real rays concentrate where the geometry is — the benchmark soup inside a room (c3d) rates PLOC 2.3 % cheaper
        // because of the room's 18 large triangles and traces 4.3 % SLOWER with it (the soup itself suits the radix tree's regular
        // cells: PLOC 4.9 % dearer, 3 % slower); a mesh gains far more than the margin (terrain: 26.5 % cheaper, 18 % fewer node
        // visits per ray, +5.5 % Mrays/s) — profiles/r4j_ploc_ab.txt, r4k_tree_costs.txt
        b.usePloc = b.opt.ploc >= 2 || cP.x < 0.95f * cR.x;
    }
    (void)hipGetLastError();
    return 0;
}

// The chosen binary tree collapsed to 4-wide nodes, one level per launch, into the BuildResult's arrays (the caller's to free).
static int collapse(Build &b, const SceneConsts *dConsts)
{
    BuildResult *out = b.out;
    const uint32_t n = b.n, nMax = (uint32_t)b.nInternal; // every 4-wide node stands for one binary inner node
    uint32_t *total; // [0] nodes appended, [1] triangles placed
    int *binOf;
    if (!(b.mem.alloc(b.finalTris, n) && b.mem.alloc(total, 2) && b.mem.alloc(binOf, nMax))) return 1;
    HR_CHECK(hipMalloc(&out->nodes, sizeof(Node4) * (size_t)nMax));
    HR_CHECK(hipMalloc(&out->nodes32, sizeof(Node32) * (size_t)nMax));
    HR_CHECK(hipMalloc(&out->leafKeys, sizeof(int) * (size_t)nMax));
    HR_CHECK(hipMalloc(&out->nodeBox, sizeof(Box6) * (size_t)nMax));
    uint32_t levelStart = 0, levelEnd = 1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const KNode *bk = b.usePloc ? b.pKnodes : b.knodes;
        const Box6 *bb = b.usePloc ? b.pBox : b.nodeBox;
        const float4 *bc = b.usePloc ? b.pCost : b.cost;
        const int rootBin = b.usePloc ? b.pRoot : 0;
        const uint32_t init[2] = {1u, 0u};
        HR_CHECK(hipMemcpyAsync(binOf, &rootBin, 4, hipMemcpyHostToDevice, b.st));
        HR_CHECK(hipMemcpyAsync(total, init, 8, hipMemcpyHostToDevice, b.st));
        levelStart = 0, levelEnd = 1;
        out->levels = 0;
        // (the radix tree is at most 58 levels deep — its key length; a PLOC tree has no such bound, so it is only kept when its collapse
        // fits the traversal stack; otherwise the second attempt collapses the radix tree)
        const int levelCap = b.usePloc ? (b.opt.maxLevels < 64 ? b.opt.maxLevels : 64) : 64;
        for (int level = 0; level < levelCap && levelEnd > levelStart; ++level) {
            const uint32_t cnt = levelEnd - levelStart;
            hipLaunchKernelGGL(k_collapse4, dim3((cnt + 255) / 256), dim3(256), 0, b.st, bk, b.leafBox, bb, binOf, levelStart, levelEnd, total, total + 1,
                               b.sorted, b.finalTris, out->nodes, out->nodeBox, dConsts, bc);
            uint32_t newEnd = 0;
            HR_CHECK(hipMemcpyAsync(&newEnd, total, 4, hipMemcpyDeviceToHost, b.st));
            HR_CHECK(hipStreamSynchronize(b.st));
            if (newEnd > nMax) return 4;
            out->levelStart[level] = levelStart, out->levelStart[level + 1] = levelEnd;
            levelStart = levelEnd;
            levelEnd = newEnd;
            out->levels = level + 1;
        }
        if (!(levelEnd > levelStart && b.usePloc)) break;
        b.usePloc = false; // too deep for the stack: fall back to the radix tree
    }
    out->builder = b.usePloc ? 1 : 0;
    if (levelEnd > levelStart) return 6; // deeper than the key length allows: cannot happen with n < 2^28
    out->nNodes = (int)levelEnd;
    uint32_t placed = 0;
    HR_CHECK(hipMemcpyAsync(&placed, total + 1, 4, hipMemcpyDeviceToHost, b.st));
    HR_CHECK(hipStreamSynchronize(b.st));
    return placed == n ? 0 : 5; // every triangle is the leaf of exactly one node
}

// the triangles in leaf order become the result's, with the way back from a prim id to its slot
static int leafOrder(Build &b)
{
    BuildResult *out = b.out;
    out->tris = b.mem.release(b.finalTris ? b.finalTris : b.sorted);
    out->triSlots = b.n;
    HR_CHECK(hipMalloc(&out->slotOfPrim, 4ull * b.n));
    hipLaunchKernelGGL(k_slot_of_prim, dim3((out->triSlots + 255) / 256), dim3(256), 0, b.st, out->tris, out->triSlots, out->slotOfPrim);
    HR_CHECK(hipStreamSynchronize(b.st));
    return hipGetLastError() != hipSuccess ? 1 : 0;
}

// Returns 0 or: 1 a HIP call failed, 2 too many triangles, 3 a refit did not reach the root, 4 / 5 / 6 the collapse made too many nodes /
// lost a triangle / is too deep, 8 more SAH work items than triangles allow (7, PLOC did not finish, never leaves: the radix tree is kept).
// The first stage that fails ends the build; the arrays of *out allocated by then are the caller's to free, like those of a finished build.
int buildLBVH(hipStream_t st, const Tri *trisPrim, uint32_t n, const float lo[3], const float hi[3], float pad, const SceneConsts *dConsts,
              BuildResult *out, const BuildOptions &opt)
{
    *out = BuildResult{};
    if (n == 0) return 0;
    if (n >= (1u << 28)) return 2;
    Build b{st, n, opt, out};
    if (int rc = sortByMorton(b, trisPrim, lo, hi, pad)) return rc;
    if (n <= 1u) { // a single triangle: the root is a leaf
        out->rootLeafCount = (int)n;
    } else {
        if (int rc = radixTree(b)) return rc;
        if (int rc = sahSubtrees(b)) return rc;
        if (int rc = plocCandidate(b)) return rc;
        if (int rc = collapse(b, dConsts)) return rc;
    }
    return leafOrder(b);
}

// ------------------------------------------------------------------------------------ content hash
// Order-independent 64-bit digest of a device buffer (words mixed with their index, then summed): the key of the tree cache.
__global__ __launch_bounds__(256) void k_hash_words(const uint32_t *__restrict__ words, size_t n, unsigned long long seed,
                                                    unsigned long long *__restrict__ out)
{
    unsigned long long acc = 0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        unsigned long long z = ((unsigned long long)words[i] << 32 | (unsigned long long)(i & 0xFFFFFFFFull)) + seed + (i >> 32) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; // splitmix64 finaliser
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        acc += z ^ (z >> 31);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
void launchHashWords(hipStream_t st, const void *words, size_t nWords, unsigned long long seed, unsigned long long *out)
{
    if (!nWords) return;
    size_t blocks = (nWords + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_hash_words, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(words), nWords, seed, out);
}

} // namespace hr
