// hr_tables.hip — the generators of the tables the renderer reads (the device side of hr_tables.h): the environment importance table and its
// guides, the mip chain with LOD scale and texel density, the QMC points, the Mersenne and blue-noise sample tables, the multiscatter LUT.
// They replace the reference's host-side generators (Source/Utility/Random.h:85-289, BlueNoise.h, Materials/MultiScatterUtil.cpp:20-139).
#include "hr_kernels.h"
#include "hr_tables.h"
#include "hr_texture.h"

namespace hr {

// ------------------------------------------------------------------ environment importance table (HR_ESTIMATOR_ENV_MIS)
// The distribution the one-sample MIS estimator draws environment directions from (include/hrcore.h): texel weight =
// (luminosity of the brightest texel of its 3 x 3 neighbourhood + maxLuminosity / 65536) x cos(elevation of the row), quantised to
// integers so that the sums do not depend on their order — the tables are bit-identical to oracle/oracle_scene.cpp::buildEnvTable.
__global__ __launch_bounds__(256) void k_env_lum(TexDesc t, float *__restrict__ lum, uint32_t *__restrict__ maxBits)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float l = 0.0f;
    if (i < (uint32_t)(t.w * t.h)) {
        const v4 c = texel(t, (int)(i % (uint32_t)t.w), (int)(i / (uint32_t)t.w));
        l = (c.x * 0.33f + c.y * 0.59f) + c.z * 0.11f; // utility.rlsl:163-166 luminosity
        l = l > 0.0f ? l : 0.0f;
        l = l < 1e30f ? l : 1e30f; // (an infinite texel must not turn the normalisation into Inf / Inf)
        lum[i] = l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l = fmax_(l, __shfl_xor(l, o));
    if ((threadIdx.x & 63) == 0 && l > 0.0f) atomicMax(maxBits, __float_as_uint(l)); // non-negative floats order like their bits
}
__global__ __launch_bounds__(256) void k_env_dilate(const float *__restrict__ lum, float *__restrict__ dil, int w, int h)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (uint32_t)(w * h)) return;
    const int i = (int)(idx % (uint32_t)w), j = (int)(idx / (uint32_t)w);
    float m = 0.0f;
    for (int dj = -1; dj <= 1; ++dj) {
        const int jj = j + dj < 0 ? 0 : (j + dj >= h ? h - 1 : j + dj);
        for (int di = -1; di <= 1; ++di) {
            const int ii = (i + di + w) % w;
            const float l = lum[(size_t)jj * w + ii];
            m = l > m ? l : m;
        }
    }
    dil[idx] = m;
}
HRD uint32_t envWeight(float lum, float floorLum, float norm, float c)
{
    const float wt = (lum + floorLum) * c;
    const float q = norm > 0.0f ? (wt / norm) * 1048576.0f : 0.0f;
    return (uint32_t)q + 1u;
}
// one workgroup per row: quantised weights and their sum
__global__ __launch_bounds__(256) void k_env_rows(const float *__restrict__ dil, int w, int h, const uint32_t *__restrict__ maxBits,
                                                  uint32_t *__restrict__ wq, unsigned long long *__restrict__ rowSum)
{
    __shared__ unsigned long long part[4];
    const int j = blockIdx.x;
    const float maxLum = __uint_as_float(*maxBits);
    const float floorLum = maxLum * (1.0f / 65536.0f), norm = maxLum + floorLum;
    const float elevation = (((float)j + 0.5f) / (float)h - 0.5f) * HR_KPI;
    const float c = cos_(elevation);
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < w; i += 256) {
        const uint32_t v = envWeight(dil[(size_t)j * w + i], floorLum, norm, c);
        wq[(size_t)j * w + i] = v;
        s += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) rowSum[j] = part[0] + part[1] + part[2] + part[3];
}
// marginal over the rows (h is at most a few thousand: one thread)
__global__ void k_env_marginal(const unsigned long long *__restrict__ rowSum, int w, int h, const uint32_t *__restrict__ maxBits,
                               float *__restrict__ rowCdf, unsigned long long *__restrict__ total, float *__restrict__ meanLum)
{
    unsigned long long t = 0;
    for (int j = 0; j < h; ++j) t += rowSum[j];
    unsigned long long acc = 0;
    for (int j = 0; j < h; ++j) {
        rowCdf[j] = (float)acc / (float)t;
        acc += rowSum[j];
    }
    rowCdf[h] = 1.0f;
    *total = t;
    // mean luminosity over the sphere from the same integers: sum(weight) / sum(cos), rows in order
    const float maxLum = __uint_as_float(*maxBits);
    const float norm = maxLum + maxLum * (1.0f / 65536.0f);
    float sumC = 0.0f;
    for (int j = 0; j < h; ++j) sumC = sumC + cos_((((float)j + 0.5f) / (float)h - 0.5f) * HR_KPI);
    *meanLum = (((float)t / 1048576.0f) * norm) / ((float)w * sumC);
}
// one workgroup per row: conditional CDF over the columns (chunked scan with a carry) and the texel probabilities
// The probability of a texel is what sampleEnv() really draws it with: the float CDF steps the two searches invert,
// (rowCdf[j + 1] - rowCdf[j]) x (colCdf[i + 1] - colCdf[i]) — not the exact ratio of the integer weights, which a float CDF of a map
// with a 2^20 : 1 weight range cannot resolve for dim texels (the balance heuristic needs the density samples are drawn with).
__global__ __launch_bounds__(256) void k_env_cols(const uint32_t *__restrict__ wq, const unsigned long long *__restrict__ rowSum,
                                                  const float *__restrict__ rowCdf, int w, float *__restrict__ colCdf,
                                                  float *__restrict__ prob)
{
    __shared__ unsigned long long waveSum[4];
    __shared__ unsigned long long carry;
    const int j = blockIdx.x;
    const float fr = (float)rowSum[j], pRow = rowCdf[j + 1] - rowCdf[j];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < w; base += 256) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long v = i < w ? (unsigned long long)wq[(size_t)j * w + i] : 0ull;
        unsigned long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o);
            if ((int)lane >= o) inc += up;
        }
        if (lane == 63) waveSum[wave] = inc;
        __syncthreads();
        unsigned long long before = carry;
        for (uint32_t k = 0; k < wave; ++k) before += waveSum[k];
        if (i < w) {
            const float cThis = (float)(before + inc - v) / fr, cNext = (i == w - 1) ? 1.0f : (float)(before + inc) / fr;
            colCdf[(size_t)j * (w + 1) + i] = cThis;
            prob[(size_t)j * w + i] = pRow * (cNext - cThis);
        }
        __syncthreads();
        if (threadIdx.x == 255) carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) colCdf[(size_t)j * (w + 1) + w] = 1.0f;
}

// scratch: lum, dil (w*h floats each), wq (w*h uint32), rowSum (h uint64), total (uint64), maxBits (uint32) — caller-owned
void launchEnvTable(hipStream_t st, const TexDesc &tex, float *lum, float *dil, uint32_t *wq, unsigned long long *rowSum, unsigned long long *total,
                    uint32_t *maxBits, float *rowCdf, float *colCdf, float *prob, float *meanLum)
{
    const int w = tex.w, h = tex.h;
    const uint32_t n = (uint32_t)((size_t)w * (size_t)h), g = (n + 255) / 256;
    hipMemsetAsync(maxBits, 0, 4, st);
    hipLaunchKernelGGL(k_env_lum, dim3(g), dim3(256), 0, st, tex, lum, maxBits);
    hipLaunchKernelGGL(k_env_dilate, dim3(g), dim3(256), 0, st, lum, dil, w, h);
    hipLaunchKernelGGL(k_env_rows, dim3(h), dim3(256), 0, st, dil, w, h, maxBits, wq, rowSum);
    hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(1), 0, st, rowSum, w, h, maxBits, rowCdf, total, meanLum);
    hipLaunchKernelGGL(k_env_cols, dim3(h), dim3(256), 0, st, wq, rowSum, rowCdf, w, colCdf, prob);
}

// Guide tables of the two inverse-CDF searches (hr_shade.h::sampleEnv): guide[k] = the largest index whose CDF value is <= k / K.
// A search for x starts in [guide[floor(x K)], guide[floor(x K) + 1]] and returns what the search over the whole table returns
// (the oracle's plain binary search), after ~2 probes instead of 10 + 11 dependent loads.
HRD int cdfSearch(const float *cdf, int lo, int hi, float x)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cdf[mid] <= x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(64) void k_env_guides(const float *__restrict__ rowCdf, const float *__restrict__ colCdf, int w, int h,
                                                   uint16_t *__restrict__ rowGuide, uint16_t *__restrict__ colGuide)
{
    // block 0: the row guide (kEnvRowGuide + 1 entries); block j + 1: the column guide of row j (kEnvColGuide + 1 entries)
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k <= kEnvRowGuide; k += 64)
            rowGuide[k] = (uint16_t)cdfSearch(rowCdf, 0, h - 1, (float)k * (1.0f / (float)kEnvRowGuide));
    } else {
        const int j = (int)blockIdx.x - 1;
        const float *cc = colCdf + (size_t)j * (w + 1);
        for (int k = threadIdx.x; k <= kEnvColGuide; k += 64)
            colGuide[(size_t)j * (kEnvColGuide + 1) + k] = (uint16_t)cdfSearch(cc, 0, w - 1, (float)k * (1.0f / (float)kEnvColGuide));
    }
}
void launchEnvGuides(hipStream_t st, const float *rowCdf, const float *colCdf, int w, int h, uint16_t *rowGuide, uint16_t *colGuide)
{
    hipLaunchKernelGGL(k_env_guides, dim3(h + 1), dim3(64), 0, st, rowCdf, colCdf, w, h, rowGuide, colGuide);
}

// ---------------------------------------------------------------------------- mip chain, texel density (HR_TEXTURE_LOD_CONE)
// One level of the chain: dst(x, y) = ((s(2x, 2y) + s(2x+1, 2y)) + (s(2x, 2y+1) + s(2x+1, 2y+1))) * 0.25 per channel, source
// coordinates clamped to the source level (odd sizes); u8 data enters as float(byte) / 255.0f, levels >= 1 are f32.
__global__ __launch_bounds__(256) void k_mip_down(const void *__restrict__ src, int srcIsU8, int sw, int sh, int c, float *__restrict__ dst, int dw, int dh)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)(dw * dh)) return;
    const int x = (int)(i % (uint32_t)dw), y = (int)(i / (uint32_t)dw);
    const int x0 = 2 * x < sw ? 2 * x : sw - 1, x1 = 2 * x + 1 < sw ? 2 * x + 1 : sw - 1;
    const int y0 = 2 * y < sh ? 2 * y : sh - 1, y1 = 2 * y + 1 < sh ? 2 * y + 1 : sh - 1;
    for (int k = 0; k < c; ++k) {
        float a, b, cc, d;
        if (srcIsU8) {
            const uint8_t *p = reinterpret_cast<const uint8_t *>(src);
            a = (float)p[((size_t)y0 * sw + x0) * c + k] / 255.0f, b = (float)p[((size_t)y0 * sw + x1) * c + k] / 255.0f;
            cc = (float)p[((size_t)y1 * sw + x0) * c + k] / 255.0f, d = (float)p[((size_t)y1 * sw + x1) * c + k] / 255.0f;
        } else {
            const float *p = reinterpret_cast<const float *>(src);
            a = p[((size_t)y0 * sw + x0) * c + k], b = p[((size_t)y0 * sw + x1) * c + k];
            cc = p[((size_t)y1 * sw + x0) * c + k], d = p[((size_t)y1 * sw + x1) * c + k];
        }
        dst[((size_t)y * dw + x) * c + k] = ((a + b) + (cc + d)) * 0.25f;
    }
}

// levels 1 .. nLevels-1 of `t` into `mips` (laid out as hr_texture.h's mipOffset expects)
void launchMipChain(hipStream_t st, const TexDesc &t, int nLevels, float *mips)
{
    const void *src = t.px;
    int srcU8 = t.dtype == HR_TEX_U8 ? 1 : 0, sw = t.w, sh = t.h;
    size_t off = 0;
    for (int l = 1; l < nLevels; ++l) {
        const int dw = sw / 2 < 1 ? 1 : sw / 2, dh = sh / 2 < 1 ? 1 : sh / 2;
        float *dst = mips + off;
        hipLaunchKernelGGL(k_mip_down, dim3(((uint32_t)(dw * dh) + 255) / 256), dim3(256), 0, st, src, srcU8, sw, sh, t.c, dst, dw, dh);
        off += (size_t)dw * dh * t.c;
        src = dst, srcU8 = 0, sw = dw, sh = dh;
    }
}

__global__ void k_tex_lod_scale(TexDesc *table, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) table[i].lodScale = 0.5f * (log_((float)table[i].w * (float)table[i].h) * 1.4426950408889634f);
}
void launchTexLodScale(hipStream_t st, TexDesc *table, int n)
{
    if (n > 0) hipLaunchKernelGGL(k_tex_lod_scale, dim3((n + 63) / 64), dim3(64), 0, st, table, n);
}

// texDensity[prim] = 0.5 * log2(uv area / world area) of every triangle (twice-areas cancel); -1e30 where either area is zero
// (no uvs, degenerate triangle): such a triangle is textured at level 0
__global__ __launch_bounds__(256) void k_tex_density(const Tri *__restrict__ leafTris, uint32_t nSlots, const TriAttr *__restrict__ attrs,
                                                     float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nSlots) return;
    const Tri tr = leafTris[i];
    const uint32_t prim = __float_as_uint(tr.r.y);
    if (prim == 0xFFFFFFFFu) return;
    const v3 e1(tr.p.w, tr.q.x, tr.q.y), e2(tr.q.z, tr.q.w, tr.r.x);
    const float world2 = length(cross(e1, e2));
    const TriAttr &a = attrs[prim];
    const float du1 = a.uv[2] - a.uv[0], dv1 = a.uv[3] - a.uv[1], du2 = a.uv[4] - a.uv[0], dv2 = a.uv[5] - a.uv[1];
    const float uv2 = abs_(du1 * dv2 - dv1 * du2);
    out[prim] = (world2 > 0.0f && uv2 > 0.0f) ? 0.5f * (log_(uv2 / world2) * 1.4426950408889634f) : -1e30f;
}
void launchTexDensity(hipStream_t st, const Tri *leafTris, uint32_t nSlots, const TriAttr *attrs, float *out)
{
    if (nSlots) hipLaunchKernelGGL(k_tex_density, dim3((nSlots + 255) / 256), dim3(256), 0, st, leafTris, nSlots, attrs, out);
}

// ---------------------------------------------------------------------------------------- QMC
// Random.h:26-34 (see oracle/oracle_qmc.cpp for the x86 conversion note)
HRD uint32_t toUint32(float f) { return (uint32_t)(unsigned long long)(long long)(f * 4294967296.0f); }
HRD float toNormalizedFloat(uint32_t u) { return (float)u * (1.0f / 4294967296.0f); }
HRD uint32_t burleyHash(uint32_t x) // Random.h:36-45
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
HRD uint32_t burleyHashCombine(uint32_t seed, uint32_t v) { return seed ^ (v + (seed << 6) + (seed >> 2)); } // :47-50
HRD uint32_t nestedUniformScramble(uint32_t x, uint32_t seed) // Random.h:52-78 (bit reversal = v_bfrev_b32)
{
    x = __brev(x);
    x += seed;
    x ^= x * 0x6c50b47cu;
    x ^= x * 0xb82f1e52u;
    x ^= x * 0xc7afe638u;
    x ^= x * 0x8d22f6e6u;
    return __brev(x);
}
HRD uint32_t sobolDim1(uint32_t index) // Random.h:236-244: v[b] = v[b-1] ^ (v[b-1] >> 1)
{
    uint32_t result = 0, v = 0x80000000u;
    for (uint32_t bit = 0; bit < 32; ++bit) {
        if ((index >> bit) & 1u) result ^= v;
        v ^= v >> 1;
    }
    return result;
}
HRD float haltonValue(uint32_t index, int base) // Random.h:192-204
{
    float result = 0.0f, f = 1.0f;
    const float denom = (float)base;
    uint32_t n = index;
    while (n > 0) {
        f = f / denom;
        result += f * (float)(n % (uint32_t)base);
        n = n / (uint32_t)base;
    }
    return result;
}
__constant__ int kHaltonBases[16][2] = {{2, 3},  {2, 5},  {2, 7},  {3, 7}, {4, 5},   {5, 7},  {5, 9},  {5, 11},
                                        {6, 11}, {5, 11}, {8, 11}, {3, 5}, {11, 15}, {2, 15}, {3, 19}, {7, 10}}; // Random.h:172-189

// owenScrambleSequence (Random.h:85-108) with sobol / halton / hammersley generators (radialSobol's disk mapping,
// Random.h:268-289, is applied on the host: hr_core.hip::radialOnHost)
__global__ __launch_bounds__(256) void k_qmc(int mode, uint32_t sequenceIndex, uint32_t count, float2 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t seed = burleyHash(sequenceIndex + 1);
    const uint32_t index = nestedUniformScramble(i, seed);
    float sx, sy;
    if (mode == HR_SAMPLE_SOBOL) {
        sx = toNormalizedFloat(__brev(index)); // dimension 0: direction numbers 2^(31-bit)
        sy = toNormalizedFloat(sobolDim1(index));
    } else if (mode == HR_SAMPLE_HALTON) {
        sx = haltonValue(index, kHaltonBases[sequenceIndex & 15][0]);
        sy = haltonValue(index, kHaltonBases[sequenceIndex & 15][1]);
    } else {
        sx = (float)i * (1.0f / (float)count);
        sy = (float)__brev(index) * 2.3283064365386963e-10f;
    }
    float x = toNormalizedFloat(nestedUniformScramble(toUint32(sx), burleyHashCombine(seed, 0)));
    float y = toNormalizedFloat(nestedUniformScramble(toUint32(sy), burleyHashCombine(seed, 1)));
    out[i] = make_float2(x, y);
}

void launchQmc(hipStream_t st, int mode, uint32_t sequenceIndex, uint32_t count, float2 *out)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_qmc, dim3((count + 255) / 256), dim3(256), 0, st, mode, sequenceIndex, count, out);
}

// ---------------------------------------------------------------- tables of the sequential generators
// util::uniformRandomFloats (edges == 0) and util::randomPolygonal (edges = 5 / 6 / 8) — Random.h:113-130, 293-355; arithmetic in hr_tables.h.
// One workgroup per sequence: MT19937's state lives in LDS, seeded by one lane (a 623-step chain), twisted by 208 lanes in three rounds
// (word i needs words i+1 and i+397 from before the twist for i < 227 and word i-227 from after it: a round of 208 < 227 words never reads a
// word of its own round after it was written) and tempered 624 draws at a time.  uniformRandomFloats maps draw 2s / 2s+1 to sample s, in parallel;
// randomPolygonal consumes a data-dependent number of draws per sample (Lemire's rejection for the fan triangle, a rejection loop for the
// barycentrics), so one lane walks the block of draws with the four-state machine of the serial loop.  The polygon's vertices come from the
// host (cosf / sinf of the platform's libm, the same calls the reference makes: like radialSobol's disk mapping in hr_scene.inl).
struct PolyVerts { float x[8], y[8]; };
static constexpr int kMtRound = 208; // 3 x 208 = 624
__global__ __launch_bounds__(256) void k_mt_tables(uint32_t seed0, uint32_t count, uint32_t edges, PolyVerts verts, float2 *__restrict__ outBase,
                                                   size_t stride)
{
    __shared__ uint32_t st[kMtN], draws[kMtN];
    __shared__ uint32_t sDone;
    const uint32_t tid = threadIdx.x;
    float2 *out = outBase + (size_t)blockIdx.x * stride;
    if (tid == 0) {
        uint32_t v = seed0 + blockIdx.x;
        st[0] = v;
        for (uint32_t i = 1; i < (uint32_t)kMtN; ++i) st[i] = v = mtSeedNext(v, i);
        sDone = 0;
    }
    __syncthreads();
    uint32_t done = 0, phase = 0; // (lane 0's: samples finished; 0 = fan triangle, first draw, 1 = its retries, 2 = alpha, 3 = beta)
    MtIntDraw pick{edges, 0u, 0ull};
    float alpha = 0.0f;
    for (uint32_t drawBase = 0;; drawBase += (uint32_t)kMtN) {
        for (int r = 0; r < 3; ++r) {
            const uint32_t i = (uint32_t)(r * kMtRound) + tid;
            uint32_t w = 0;
            if (tid < (uint32_t)kMtRound) w = mtTwist(st[i], st[(i + 1) % kMtN], st[(i + kMtM) % kMtN]);
            __syncthreads();
            if (tid < (uint32_t)kMtRound) st[i] = w;
            __syncthreads();
        }
        for (uint32_t k = tid; k < (uint32_t)kMtN; k += 256) draws[k] = mtTemper(st[k]);
        __syncthreads();
        if (edges == 0) {
            float *o = reinterpret_cast<float *>(out);
            for (uint32_t k = tid; k < (uint32_t)kMtN; k += 256) {
                const uint64_t g = (uint64_t)drawBase + k;
                if (g < 2ull * count) o[g] = mtCanonical(draws[k]);
            }
            if ((uint64_t)drawBase + kMtN >= 2ull * count) break;
        } else {
            if (tid == 0) {
                for (int k = 0; k < kMtN && done < count; ++k) {
                    const uint32_t u = draws[k];
                    if (phase < 2) {
                        phase = pick.accept(u, phase == 0) ? 2u : 1u;
                    } else if (phase == 2) {
                        alpha = mtCanonical(u), phase = 3;
                    } else {
                        const float beta = mtCanonical(u);
                        if (alpha + beta > 1.0f) {
                            phase = 2;
                            continue;
                        }
                        const float gamma = 1.0f - (alpha + beta);
                        const int t0 = pick.value(), t1 = (t0 + 1) % (int)edges;
                        const float vx = 0.0f * alpha + verts.x[t0] * beta + verts.x[t1] * gamma; // (the fan's centre is vertex 0 of every triangle)
                        const float vy = 0.0f * alpha + verts.y[t0] * beta + verts.y[t1] * gamma;
                        out[done++] = make_float2((vx + 1.0f) * 0.5f, (vy + 1.0f) * 0.5f);
                        phase = 0;
                    }
                }
                sDone = done;
            }
            __syncthreads();
            if (sDone >= count) break;
        }
    }
}
void launchMtTables(hipStream_t st, uint32_t seed0, int nSeq, uint32_t count, uint32_t edges, const float *vx, const float *vy, float2 *out, size_t stride)
{
    if (count == 0 || nSeq <= 0) return;
    PolyVerts v{};
    for (uint32_t i = 0; i < edges && i < 8u; ++i) v.x[i] = vx[i], v.y[i] = vy[i];
    hipLaunchKernelGGL(k_mt_tables, dim3((uint32_t)nSeq), dim3(256), 0, st, seed0, count, edges, v, out, stride);
}

// util::blueNoise (BlueNoise.h:52-88): point i is the best of 30 hashed candidates, "best" = furthest from its nearest earlier point.  The
// candidates do not depend on the points (a hash of a running seed), so one launch makes them all; the choice is sequential over the points
// and parallel inside a point: a workgroup per sequence, 30 groups of 32 lanes — a group per candidate, a lane per 32nd earlier point —
// min over squared distances (the square root is monotone, it is taken once per candidate), then one lane picks the first candidate whose
// nearest distance exceeds the running maximum, as the serial loop does.  15 n^2 distance tests per sequence of n points.
static constexpr int kBlueCandidates = 30, kBlueLds = 8192;
__global__ __launch_bounds__(256) void k_blue_candidates(int32_t seq0, uint32_t nSeq, uint32_t count, float2 *__restrict__ cand, float2 *__restrict__ outBase, size_t stride)
{
    const uint32_t perSeq = (count - 1u) * (uint32_t)kBlueCandidates + 1u; // (entry 0: the first point itself)
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t s = (uint32_t)(gid / perSeq), k = (uint32_t)(gid % perSeq);
    if (s >= nSeq) return;
    const uint32_t seed = blueSeed(seq0 + (int32_t)s) + 2u * k;
    const float2 p = make_float2(blueRandom(seed), blueRandom(seed + 1u));
    if (k == 0)
        outBase[(size_t)s * stride] = p;
    else
        cand[(size_t)s * (perSeq - 1u) + (k - 1u)] = p;
}
template <bool LDS>
__global__ __launch_bounds__(1024) void k_blue_noise(uint32_t count, const float2 *__restrict__ candBase, float2 *__restrict__ outBase, size_t stride)
{
    __shared__ float2 ptsLds[LDS ? kBlueLds : 1];
    __shared__ float nearest[32];
    float2 *out = outBase + (size_t)blockIdx.x * stride;
    const float2 *cand = candBase + (size_t)blockIdx.x * (count - 1u) * kBlueCandidates;
    float2 *pts = LDS ? ptsLds : out;
    const uint32_t tid = threadIdx.x, g = tid >> 5, l = tid & 31u;
    if (LDS && tid == 0) ptsLds[0] = out[0];
    __syncthreads();
    const float diag = sqrt_(1.0f * 1.0f + 1.0f * 1.0f);
    for (uint32_t i = 1; i < count; ++i) {
        if (g < (uint32_t)kBlueCandidates) {
            const float2 c = cand[(size_t)(i - 1u) * kBlueCandidates + g];
            float m = 3.0e38f;
            for (uint32_t j = l; j < i; j += 32u) {
                const float2 p = pts[j];
                const float dx = p.x - c.x, dy = p.y - c.y;
                m = fmin_(m, dx * dx + dy * dy);
            }
#pragma unroll
            for (int sh = 16; sh > 0; sh >>= 1) m = fmin_(m, __shfl_xor(m, sh));
            if (l == 0) nearest[g] = fmin_(diag, sqrt_(m));
        }
        __syncthreads();
        if (tid == 0) {
            float furthest = 0.0f;
            int best = -1;
            for (int c = 0; c < kBlueCandidates; ++c)
                if (nearest[c] > furthest) furthest = nearest[c], best = c;
            const float2 p = best < 0 ? make_float2(0.0f, 0.0f) : cand[(size_t)(i - 1u) * kBlueCandidates + best];
            pts[i] = p;
            if (LDS) out[i] = p;
        }
        __syncthreads();
    }
}
// cand: scratch of nSeq * (count - 1) * 30 points
void launchBlueNoise(hipStream_t st, int32_t seq0, int nSeq, uint32_t count, float2 *out, size_t stride, float2 *cand)
{
    if (count == 0 || nSeq <= 0) return;
    const uint64_t total = (uint64_t)nSeq * ((uint64_t)(count - 1u) * kBlueCandidates + 1u);
    hipLaunchKernelGGL(k_blue_candidates, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, seq0, (uint32_t)nSeq, count, cand, out, stride);
    int dev = 0, ldsMax = 0; // (the LDS copy of the points is 64 KB + the candidates' row: more than a gfx9 before gfx950 gives one workgroup)
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ldsMax, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) ldsMax = 0;
    if (count <= (uint32_t)kBlueLds && (size_t)ldsMax >= sizeof(float2) * kBlueLds + 256)
        hipLaunchKernelGGL(k_blue_noise<true>, dim3((uint32_t)nSeq), dim3(1024), 0, st, count, cand, out, stride);
    else
        hipLaunchKernelGGL(k_blue_noise<false>, dim3((uint32_t)nSeq), dim3(1024), 0, st, count, cand, out, stride);
}

// ------------------------------------------------------------------------------ multiscatter LUT
// MultiScatterUtil.cpp:20-139: one thread per texel integrates 4096 Sobol samples of the GGX lobe.
HRD float lutG1(float NdotI, float alpha)
{
    const float alpha2 = alpha * alpha;
    const float denom = sqrt_(alpha2 + (1.0f - alpha2) * (NdotI * NdotI)) + NdotI;
    return (2.0f * NdotI) / fmax_(denom, 1e-5f);
}
__global__ __launch_bounds__(128) void k_multiscatter_lut(const float2 *__restrict__ seq, int samples, float *__restrict__ out, int dim)
{
    const int col = threadIdx.x, row = blockIdx.x;
    const float roughness = clamp_(((float)row + 0.5f) / (float)dim, 0.0f, 1.0f);
    const float alpha = roughness * roughness;
    const float NdotV = clamp_(((float)col + 0.5f) / (float)dim, 0.0f, 1.0f);
    const v3 V(sqrt_(1.0f - (NdotV * NdotV)), 0.0f, NdotV);
    float result = 0.0f;
    for (int i = 0; i < samples; ++i) {
        const float2 r = seq[i];
        const float a2 = alpha * alpha;
        const float cosTheta = sqrt_(fmax_(0.0f, (1.0f - r.x) / ((a2 - 1.0f) * r.x + 1.0f)));
        const float sinTheta = sqrt_(fmax_(0.0f, 1.0f - cosTheta * cosTheta));
        float sn, cs;
        sincos_(6.28318530717958647692f * r.y, &sn, &cs);
        v3 H(sinTheta * cs, sinTheta * sn, cosTheta);
        H = normalize(H);
        const v3 L = 2.0f * dot(V, H) * H - V;
        const float NdotL = clamp_(L.z, 0.0f, 1.0f);
        if (NdotL > 0.0f) {
            const float VdotH = clamp_(dot(V, H), 0.0f, 1.0f);
            const float NdotH = clamp_(H.z, 0.0f, 1.0f);
            result += (lutG1(NdotL, alpha) * lutG1(NdotV, alpha) * VdotH) / (NdotV * NdotH);
        }
    }
    const float value = result / (float)samples;
    out[row * dim + col] = (1.0f - value) / value;
}

void launchMultiscatterLUT(hipStream_t st, const float2 *sobol4096, float *out128x128)
{
    hipLaunchKernelGGL(k_multiscatter_lut, dim3(128), dim3(128), 0, st, sobol4096, 4096, out128x128, 128);
}

} // namespace hr
