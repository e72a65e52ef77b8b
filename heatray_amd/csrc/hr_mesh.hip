// hr_mesh.hip — the kernels of mesh preparation (include/hrcore_mesh.h is the contract, hr_mesh.h the per-element arithmetic,
// hr_mesh.inl the entry points).  A translation unit of its own.  A scatter-sum whose result must be the same bits on every run: no
// float atomics; every contribution is stored once and summed per destination through an inverted index, in one fixed order.
//
//   k_mesh_face      one lane per triangle: the face terms, the three corners' contributions (normal; tangent and bitangent when wanted)
//                    with plain stores, the triangle's flags, and the corner sort's input (key = the corner's vertex, value = the corner).
//                    Counts the degenerate classes per wave (hr_post_device.h).
//   k_mesh_sort_hist, k_mesh_scan, k_mesh_sort_scatter
//                    a stable LSD radix sort of (key, value) pairs by 8-bit digits, the shape of hr_build.hip's: per-tile digit
//                    histograms, ONE workgroup scans them (a launch of its own: no kernel waits on another workgroup's progress), a
//                    ballot-ranked scatter.  Equal keys keep their order, so a vertex's corners stay in ascending corner index and a
//                    position group's vertices in ascending vertex index: the contract's orders.  Digit passes above the highest set bit
//                    of n_vertices - 1 are skipped for the corner sort.
//   k_mesh_ranges    sorted corners -> every vertex's range in them (the first and one past the last place its key stands at)
//   k_mesh_iota, k_mesh_weld_keys, k_mesh_heads, k_mesh_groups
//                    the weld: the vertex ids sorted by the ordered-float keys of z, then y, then x (positions + 0.0f: -0 is +0); a run's
//                    head differs from its predecessor; the scan of the heads numbers the groups.  weld = 0: k_mesh_iota alone makes
//                    every vertex its own group.
//   k_mesh_vertex    one lane per vertex: walks its corners, writes S, Ta, Ba and its lowest non-degenerate corner; the longest list
//   k_mesh_group     one lane per group: walks its members, writes the group's normal and what became of it
//   k_mesh_finish    one lane per vertex: the outputs (12 bytes per lane and array, consecutive lanes consecutive: coalesced) and the
//                    three vertex counters
// Indices are 32-bit where they count corners or vertices (at most 2^32 - 1 corners: the host refuses more) and size_t where they
// address floats.  Every index read from the caller's buffer has been checked against n_vertices on the host before the first launch.
#include "hr_math.h"
#include "hr_mesh.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kMsBlock = 256;      // lanes per workgroup of the per-triangle, per-vertex and per-group kernels
static constexpr int kMsSortTile = 2048;  // keys per single-wave workgroup of the sort
static constexpr int kMsScanBlock = 1024; // lanes of the scan's one workgroup
static constexpr int kMsScanPer = 4;      // ... and the values each takes per round

HRD uint32_t msOrdered(float f)
{
    const uint32_t b = __float_as_uint(f + 0.0f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
HRD v3 msLoad3(const float *a, uint32_t i)
{
    const HR_GLOBAL float *p = G(a) + 3 * (size_t)i;
    return v3(p[0], p[1], p[2]);
}
HRD void msStore3(float *a, size_t i, v3 v)
{
    HR_GLOBAL float *p = G(a) + 3 * i;
    p[0] = v.x, p[1] = v.y, p[2] = v.z;
}

// ------------------------------------------------------------------------------------------ faces
__global__ __launch_bounds__(kMsBlock) void k_mesh_face(MsBufs b)
{
    __shared__ uint32_t sRed[2];
    wgCountersZero<2>(sRed);
    __syncthreads();
    const uint32_t t = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    const bool in = t < b.T;
    bool degenerate = false, degenerateUv = false;
    if (in) {
        uint32_t id[3];
        msTriangle(G(b.idx), t, b.strip != 0, id);
        const v3 p0 = msLoad3(b.pos, id[0]), p1 = msLoad3(b.pos, id[1]), p2 = msLoad3(b.pos, id[2]);
        v3 e1, e2, u;
        float w[3];
        const bool face = msFace(p0, p1, p2, b.weight, e1, e2, u, w);
        degenerate = !face;
        const size_t c0 = 3 * (size_t)t;
        uint32_t flags = face ? MS_FACE : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            msStore3(b.cN, c0 + k, u * w[k]); // (a DEGENERATE triangle: 0 0 0, and its flag keeps the corner out of every sum)
            G(b.keysA)[c0 + k] = id[k];
            G(b.valsA)[c0 + k] = (uint32_t)(c0 + k);
        }
        if (b.want & HR_MESH_WANT_TANGENTS) {
            v3 Tn(0.0f), Bn(0.0f);
            if (face) {
                const HR_GLOBAL float *q0 = G(b.uv) + 2 * (size_t)id[0], *q1 = G(b.uv) + 2 * (size_t)id[1], *q2 = G(b.uv) + 2 * (size_t)id[2];
                const bool uvOk = msFaceTangents(e1, e2, q0[0], q0[1], q1[0], q1[1], q2[0], q2[1], Tn, Bn);
                degenerateUv = !uvOk;
                flags |= uvOk ? MS_UV : 0;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                msStore3(b.cT, c0 + k, Tn * w[k]);
                msStore3(b.cB, c0 + k, Bn * w[k]);
            }
        }
        G(b.tflag)[t] = (uint8_t)flags;
    }
    const uint32_t nDeg = waveCount(degenerate), nDegUv = waveCount(degenerateUv);
    if ((threadIdx.x & 63u) == 0u) {
        if (nDeg) atomicAdd(&sRed[0], nDeg);
        if (nDegUv) atomicAdd(&sRed[1], nDegUv);
    }
    wgCountersFlush<2>(sRed, b.counters + kMsDegenerate);
}

// ------------------------------------------------------------------------------------------ radix sort
__global__ __launch_bounds__(64) void k_mesh_sort_hist(const uint32_t *__restrict__ keys, uint32_t n, int shift, uint32_t *__restrict__ blockHist, uint32_t nBlocks)
{
    __shared__ uint32_t hist[256];
    for (int i = threadIdx.x; i < 256; i += 64) hist[i] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * kMsSortTile;
    for (int r = 0; r < kMsSortTile / 64; ++r) {
        const unsigned long long i = base + (uint32_t)(r * 64) + threadIdx.x;
        if (i < n) atomicAdd(&hist[(G(keys)[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += 64) G(blockHist)[(size_t)i * nBlocks + blockIdx.x] = hist[i];
}

// exclusive scan of n values in place by ONE workgroup; `total`, where not null, gets their sum
__global__ __launch_bounds__(kMsScanBlock) void k_mesh_scan(uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ total)
{
    __shared__ uint32_t waveSums[kMsScanBlock / 64];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long base = 0; base < n; base += (uint32_t)(kMsScanBlock * kMsScanPer)) {
        const unsigned long long i0 = base + (unsigned long long)threadIdx.x * kMsScanPer;
        uint32_t v[kMsScanPer], s = 0;
#pragma unroll
        for (int k = 0; k < kMsScanPer; ++k) {
            v[k] = (i0 + k < n) ? G(data)[i0 + k] : 0u;
            s += v[k];
        }
        uint32_t inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o);
            if ((int)lane >= o) inc += up;
        }
        if (lane == 63u) waveSums[wave] = inc;
        __syncthreads();
        uint32_t wavePrefix = 0;
        for (uint32_t w = 0; w < wave; ++w) wavePrefix += waveSums[w];
        const uint32_t c = carry;
        uint32_t ex = c + wavePrefix + inc - s;
#pragma unroll
        for (int k = 0; k < kMsScanPer; ++k) {
            if (i0 + k < n) G(data)[i0 + k] = ex;
            ex += v[k];
        }
        __syncthreads();
        if (threadIdx.x == kMsScanBlock - 1) carry = ex;
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) *G(total) = carry;
}

__global__ __launch_bounds__(64) void k_mesh_sort_scatter(const uint32_t *__restrict__ keysIn, const uint32_t *__restrict__ valsIn, uint32_t n, int shift,
                                                          const uint32_t *__restrict__ blockOffsets, uint32_t nBlocks, uint32_t *__restrict__ keysOut,
                                                          uint32_t *__restrict__ valsOut)
{
    __shared__ uint32_t off[256];
    for (int i = threadIdx.x; i < 256; i += 64) off[i] = G(blockOffsets)[(size_t)i * nBlocks + blockIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x;
    const unsigned long long ltMask = (1ull << lane) - 1ull;
    const unsigned long long base = (unsigned long long)blockIdx.x * kMsSortTile;
    for (int r = 0; r < kMsSortTile / 64; ++r) {
        const unsigned long long i = base + (uint32_t)(r * 64) + lane;
        const bool valid = i < n;
        const uint32_t key = valid ? G(keysIn)[i] : 0u, val = valid ? G(valsIn)[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        // lanes holding the same digit (stable: rank = the equal-digit lanes before this one)
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1u;
            const unsigned long long m = __ballot(set);
            same &= set ? m : ~m;
        }
        uint32_t pos = 0;
        if (valid) pos = off[d] + (uint32_t)__popcll(same & ltMask); // (< n: the offsets are the scanned counts of exactly these keys)
        __syncthreads();
        if (valid && (same & ltMask) == 0ull) off[d] += (uint32_t)__popcll(same); // the first lane of each digit's lanes
        __syncthreads();
        if (valid) {
            G(keysOut)[pos] = key;
            G(valsOut)[pos] = val;
        }
    }
}

// ------------------------------------------------------------------------------------------ the inverted index
// keys: the C corners' vertices, sorted; vBegin / vEnd zeroed by the caller (a vertex nobody names keeps the empty range 0 .. 0)
__global__ __launch_bounds__(kMsBlock) void k_mesh_ranges(const uint32_t *__restrict__ keys, uint32_t C, uint32_t *__restrict__ vBegin, uint32_t *__restrict__ vEnd)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= C) return;
    const uint32_t k = G(keys)[i];
    if (i == 0 || G(keys)[i - 1] != k) G(vBegin)[k] = (uint32_t)i;
    if (i + 1 == C || G(keys)[i + 1] != k) G(vEnd)[k] = (uint32_t)(i + 1); // (C <= 2^32 - 1: no wrap)
}

// ------------------------------------------------------------------------------------------ weld
// vals[i] = i; with `identity` also every vertex as its own group
__global__ __launch_bounds__(kMsBlock) void k_mesh_iota(MsBufs b, uint32_t *__restrict__ vals, int identity)
{
    const uint32_t i = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    if (i >= b.V) return;
    G(vals)[i] = i;
    if (identity) {
        G(b.groupOf)[i] = i, G(b.groupStart)[i] = i;
        if (i == b.V - 1u) G(b.groupStart)[b.V] = b.V, *G(b.nGroups) = b.V, G(b.counters)[kMsGroups] = b.V;
    }
}

__global__ __launch_bounds__(kMsBlock) void k_mesh_weld_keys(const float *__restrict__ pos, uint32_t V, int axis, const uint32_t *__restrict__ vals, uint32_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    if (i >= V) return;
    G(keys)[i] = msOrdered(G(pos)[3 * (size_t)G(vals)[i] + axis]);
}

HRD bool msHead(const float *pos, const uint32_t *perm, uint32_t i)
{
    if (i == 0u) return true;
    const v3 a = msLoad3(pos, G(perm)[i]), p = msLoad3(pos, G(perm)[i - 1]);
    return !(a.x == p.x && a.y == p.y && a.z == p.z);
}

__global__ __launch_bounds__(kMsBlock) void k_mesh_heads(MsBufs b, const uint32_t *__restrict__ perm)
{
    const uint32_t i = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    if (i >= b.V) return;
    G(b.scan)[i] = msHead(b.pos, perm, i) ? 1u : 0u;
}

// b.scan: the exclusive scan of the heads
__global__ __launch_bounds__(kMsBlock) void k_mesh_groups(MsBufs b, const uint32_t *__restrict__ perm)
{
    const uint32_t i = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    if (i >= b.V) return;
    const bool head = msHead(b.pos, perm, i);
    const uint32_t g = G(b.scan)[i] + (head ? 1u : 0u) - 1u; // (place 0 is a head: never below 0)
    G(b.groupOf)[G(perm)[i]] = g;
    if (head) G(b.groupStart)[g] = i;
    if (i == b.V - 1u) G(b.groupStart)[g + 1u] = b.V, *G(b.nGroups) = g + 1u, G(b.counters)[kMsGroups] = g + 1u;
}

// ------------------------------------------------------------------------------------------ the sums
// corners: the corner ids sorted by vertex
__global__ __launch_bounds__(kMsBlock) void k_mesh_vertex(MsBufs b, const uint32_t *__restrict__ corners)
{
    __shared__ uint32_t sMax;
    if (threadIdx.x == 0) sMax = 0u;
    __syncthreads();
    const uint32_t v = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    uint32_t valence = 0;
    if (v < b.V) {
        const uint32_t begin = G(b.vBegin)[v], end = G(b.vEnd)[v];
        valence = end - begin;
        const bool tangents = (b.want & HR_MESH_WANT_TANGENTS) != 0;
        v3 S(0.0f), Ta(0.0f), Ba(0.0f);
        uint32_t first = kMsNoCorner;
        for (uint32_t i = begin; i < end; ++i) {
            const uint32_t c = G(corners)[i];
            const uint32_t f = G(b.tflag)[c / 3u];
            if (f & MS_FACE) {
                S = S + msLoad3(b.cN, c);
                first = first == kMsNoCorner ? c : first; // (ascending: the first one met is the lowest)
            }
            if (tangents && (f & MS_UV)) {
                Ta = Ta + msLoad3(b.cT, c);
                Ba = Ba + msLoad3(b.cB, c);
            }
        }
        msStore3(b.vS, v, S);
        G(b.vFirst)[v] = first;
        if (tangents) msStore3(b.vTa, v, Ta), msStore3(b.vBa, v, Ba);
    }
    uint32_t m = valence;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63u) == 0u && m) atomicMax(&sMax, m);
    __syncthreads();
    if (threadIdx.x == 0 && sMax) atomicMax(&b.counters[kMsMaxValence], (unsigned long long)sMax);
}

__global__ __launch_bounds__(kMsBlock) void k_mesh_group(MsBufs b, const uint32_t *__restrict__ perm)
{
    const uint32_t g = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    if (g >= *G(b.nGroups)) return;
    const uint32_t begin = G(b.groupStart)[g], end = G(b.groupStart)[g + 1u];
    v3 Gs(0.0f);
    uint32_t first = kMsNoCorner;
    for (uint32_t j = begin; j < end; ++j) {
        const uint32_t v = G(perm)[j];
        Gs = Gs + msLoad3(b.vS, v);
        const uint32_t f = G(b.vFirst)[v];
        first = f < first ? f : first;
    }
    v3 uFirst(0.0f);
    if (first != kMsNoCorner && !msValid(dot(Gs, Gs))) {
        uint32_t id[3];
        msTriangle(G(b.idx), first / 3u, b.strip != 0, id);
        uFirst = msFaceUnit(msLoad3(b.pos, id[0]), msLoad3(b.pos, id[1]), msLoad3(b.pos, id[2]));
    }
    v3 N;
    const int cls = msFinishNormal(Gs, first, uFirst, N);
    msStore3(b.gN, g, N);
    G(b.gClass)[g] = (uint8_t)cls;
}

__global__ __launch_bounds__(kMsBlock) void k_mesh_finish(MsBufs b)
{
    __shared__ uint32_t sRed[3];
    wgCountersZero<3>(sRed);
    __syncthreads();
    const uint32_t v = blockIdx.x * (uint32_t)kMsBlock + threadIdx.x;
    bool unreferenced = false, cancelled = false, fallback = false;
    if (v < b.V) {
        v3 N;
        bool haveN;
        if (b.want & HR_MESH_WANT_NORMALS) {
            const uint32_t g = G(b.groupOf)[v];
            N = msLoad3(b.gN, g);
            const int cls = G(b.gClass)[g];
            unreferenced = cls == MS_UNREFERENCED, cancelled = cls == MS_CANCELLED;
            haveN = !unreferenced;
            msStore3(b.outN, v, N);
        } else {
            haveN = msGivenNormal(msLoad3(b.nrmIn, v), N);
        }
        if (b.want & HR_MESH_WANT_TANGENTS) {
            v3 tangent, bitangent;
            fallback = msFinishTangent(haveN, N, msLoad3(b.vTa, v), msLoad3(b.vBa, v), tangent, bitangent);
            msStore3(b.outT, v, tangent);
            msStore3(b.outB, v, bitangent);
        }
    }
    const uint32_t nU = waveCount(unreferenced), nC = waveCount(cancelled), nF = waveCount(fallback);
    if ((threadIdx.x & 63u) == 0u) {
        if (nU) atomicAdd(&sRed[0], nU);
        if (nC) atomicAdd(&sRed[1], nC);
        if (nF) atomicAdd(&sRed[2], nF);
    }
    wgCountersFlush<3>(sRed, b.counters + kMsUnreferenced);
}

// ------------------------------------------------------------------------------------------ host
static uint32_t msGrid(uint32_t n) { return (n + (uint32_t)kMsBlock - 1u) / (uint32_t)kMsBlock; }

size_t meshSortBlocks(size_t n) { return (n + kMsSortTile - 1) / kMsSortTile; }

// (keys, vals) of n pairs in keysA / valsA sorted by the low `passes` bytes of the keys; the sorted arrays' pointers come back in place
static void msSort(hipStream_t st, const MsBufs &b, uint32_t n, int passes, uint32_t *&keysA, uint32_t *&valsA, uint32_t *&keysB, uint32_t *&valsB)
{
    const uint32_t nBlocks = (uint32_t)meshSortBlocks(n);
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = pass * 8;
        hipLaunchKernelGGL(k_mesh_sort_hist, dim3(nBlocks), dim3(64), 0, st, keysA, n, shift, b.blockHist, nBlocks);
        hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMsScanBlock), 0, st, b.blockHist, 256u * nBlocks, (uint32_t *)nullptr);
        hipLaunchKernelGGL(k_mesh_sort_scatter, dim3(nBlocks), dim3(64), 0, st, keysA, valsA, n, shift, b.blockHist, nBlocks, keysB, valsB);
        std::swap(keysA, keysB);
        std::swap(valsA, valsB);
    }
}

// Everything between the uploads and the copies back, on `st`.  The caller has zeroed b.counters.
void launchMeshPrepare(hipStream_t st, const MsBufs &b)
{
    const bool normals = (b.want & HR_MESH_WANT_NORMALS) != 0;
    uint32_t *keysA = b.keysA, *keysB = b.keysB, *valsA = b.valsA, *valsB = b.valsB;
    (void)hipMemsetAsync(b.vBegin, 0, (size_t)b.V * 4, st);
    (void)hipMemsetAsync(b.vEnd, 0, (size_t)b.V * 4, st);
    if (b.T) {
        hipLaunchKernelGGL(k_mesh_face, dim3(msGrid(b.T)), dim3(kMsBlock), 0, st, b);
        // the digit passes the vertex ids need: none above the highest set bit of V - 1
        int bits = 0;
        while (bits < 32 && ((b.V - 1u) >> bits) != 0u) ++bits;
        msSort(st, b, b.C, (bits + 7) / 8, keysA, valsA, keysB, valsB);
        hipLaunchKernelGGL(k_mesh_ranges, dim3((uint32_t)(((size_t)b.C + kMsBlock - 1) / kMsBlock)), dim3(kMsBlock), 0, st, keysA, b.C, b.vBegin, b.vEnd);
    }
    uint32_t *corners = valsA; // (stays where it is: the weld sorts in the other three arrays and b.perm)
    hipLaunchKernelGGL(k_mesh_vertex, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b, corners);
    if (normals) {
        uint32_t *wKeysA = keysA, *wKeysB = keysB, *wValsA = b.perm, *wValsB = valsB;
        hipLaunchKernelGGL(k_mesh_iota, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b, wValsA, b.weld ? 0 : 1);
        if (b.weld) {
            for (int axis = 2; axis >= 0; --axis) {
                hipLaunchKernelGGL(k_mesh_weld_keys, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b.pos, b.V, axis, wValsA, wKeysA);
                msSort(st, b, b.V, 4, wKeysA, wValsA, wKeysB, wValsB);
            }
            hipLaunchKernelGGL(k_mesh_heads, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b, wValsA);
            hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMsScanBlock), 0, st, b.scan, b.V, (uint32_t *)nullptr);
            hipLaunchKernelGGL(k_mesh_groups, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b, wValsA);
        }
        hipLaunchKernelGGL(k_mesh_group, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b, wValsA);
    }
    hipLaunchKernelGGL(k_mesh_finish, dim3(msGrid(b.V)), dim3(kMsBlock), 0, st, b);
}

} // namespace hr
