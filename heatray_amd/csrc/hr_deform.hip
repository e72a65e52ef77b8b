// hr_deform.hip — the kernels of deformable meshes (include/hrcore_deform.h is the contract, hr_deform.h the per-vertex arithmetic,
// hr_deform.inl the entry points).  A translation unit of its own.  A mesh block keeps its attributes as the caller handed them over,
// each with its own stride; everything that computes works on TIGHT arrays (3 floats per vertex, 2 for uvs), so the three kernels are
//
//   k_deform_gather   strided block -> tight arrays, up to four attributes per launch, one lane per vertex: the rest snapshot of a
//                     bind, the read-back, and the inputs of a regeneration
//   k_deform_pose     one lane per vertex, tight in, tight out: consecutive lanes read and write consecutive 12-byte records.  The
//                     morph weights and the joint matrices (64 bytes per joint, 64 KB at most) are read through the cache: every
//                     workgroup reads the same few KB, and neighbouring vertices mostly name the same joints.  Position, normal,
//                     tangent and bitangent are posed ONE AFTER THE OTHER, each stored before the next begins (they are independent
//                     sums): 42 VGPRs, where all four in flight joint by joint took 76.  The price is that a vertex's weights, joint
//                     indices and matrices are read once per output, from the cache.  Counts per wave.
//   k_deform_scatter  tight arrays -> the block's strided slots, up to four attributes per launch: shared by update and pose
//
// Vertex indices are 32-bit, addresses size_t.  No index read from memory addresses anything unchecked: hr_deform_bind has checked
// every joint index against n_joints on the host.  The strided side of a copy lies inside the block by hr_geom_add's layout:
// offset + (V - 1) * stride + comps floats.
#include "hr_math.h"
#include "hr_deform.h"
#include "hr_kernels.h"
#include "hr_post_device.h"

namespace hr {

static constexpr int kDfBlock = 256; // lanes per workgroup of all three kernels

__global__ __launch_bounds__(kDfBlock) void k_deform_gather(DfCopy s)
{
    const uint32_t v = blockIdx.x * (uint32_t)kDfBlock + threadIdx.x;
    if (v >= s.V) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a >= s.n) break;
        const HR_GLOBAL float *src = G(s.strided[a]) + (size_t)v * (size_t)s.stride[a];
        HR_GLOBAL float *dst = G(s.tight[a]) + (size_t)v * (size_t)s.comps[a];
        dst[0] = src[0], dst[1] = src[1];
        if (s.comps[a] == 3) dst[2] = src[2];
    }
}

__global__ __launch_bounds__(kDfBlock) void k_deform_scatter(DfCopy s)
{
    const uint32_t v = blockIdx.x * (uint32_t)kDfBlock + threadIdx.x;
    if (v >= s.V) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a >= s.n) break;
        const HR_GLOBAL float *src = G((const float *)s.tight[a]) + (size_t)v * (size_t)s.comps[a];
        HR_GLOBAL float *dst = G(s.strided[a]) + (size_t)v * (size_t)s.stride[a];
        dst[0] = src[0], dst[1] = src[1];
        if (s.comps[a] == 3) dst[2] = src[2];
    }
}

HRD void dfStore3(float *a, uint32_t v, v3 x)
{
    HR_GLOBAL float *p = G(a) + 3 * (size_t)v;
    p[0] = x.x, p[1] = x.y, p[2] = x.z;
}

__global__ __launch_bounds__(kDfBlock) void k_deform_pose(DfPoseArgs s)
{
    __shared__ uint32_t sRed[2];
    wgCountersZero<2>(sRed);
    __syncthreads();
    const uint32_t v = blockIdx.x * (uint32_t)kDfBlock + threadIdx.x;
    uint32_t rejected = 0, kept = 0;
    if (v < s.V) {
        DfRig<const HR_GLOBAL float *, const HR_GLOBAL uint32_t *> r;
        r.dP = G(s.dP), r.dN = G(s.dN), r.joints = G(s.joints), r.weights = G(s.weights), r.morphW = G(s.pose), r.mats = G(s.pose) + HR_DEFORM_MAX_MORPH;
        r.V = s.V, r.nMorph = s.nMorph, r.nJoints = s.nJoints;
        bool keep;
        dfStore3(s.outP, v, dfPosePosition(r, v, dfLoad3(G(s.restP), v), keep));
        rejected = keep ? 1u : 0u;
        // (each output is stored before the next is begun: see hr_deform.h)
        if (s.outN) dfStore3(s.outN, v, dfPoseNormal(r, v, dfLoad3(G(s.restN), v), keep)), kept += keep ? 1u : 0u;
        if (s.outT) {
            dfStore3(s.outT, v, dfPoseFrame(r, v, dfLoad3(G(s.restT), v), keep)), kept += keep ? 1u : 0u;
            dfStore3(s.outB, v, dfPoseFrame(r, v, dfLoad3(G(s.restB), v), keep)), kept += keep ? 1u : 0u;
        }
    }
    const uint32_t nR = waveSum(rejected), nK = waveSum(kept);
    if ((threadIdx.x & 63u) == 0u) {
        if (nR) atomicAdd(&sRed[0], nR);
        if (nK) atomicAdd(&sRed[1], nK);
    }
    wgCountersFlush<2>(sRed, s.counters);
}

// ------------------------------------------------------------------------------------------ host
static uint32_t dfGrid(uint32_t n) { return (n + (uint32_t)kDfBlock - 1u) / (uint32_t)kDfBlock; }

void launchDeformGather(hipStream_t st, const DfCopy &s)
{
    if (s.V && s.n) hipLaunchKernelGGL(k_deform_gather, dim3(dfGrid(s.V)), dim3(kDfBlock), 0, st, s);
}
void launchDeformScatter(hipStream_t st, const DfCopy &s)
{
    if (s.V && s.n) hipLaunchKernelGGL(k_deform_scatter, dim3(dfGrid(s.V)), dim3(kDfBlock), 0, st, s);
}
void launchDeformPose(hipStream_t st, const DfPoseArgs &s)
{
    if (s.V) hipLaunchKernelGGL(k_deform_pose, dim3(dfGrid(s.V)), dim3(kDfBlock), 0, st, s);
}

} // namespace hr
