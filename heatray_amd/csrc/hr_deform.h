// hr_deform.h — the per-vertex arithmetic of hr_deform_pose (include/hrcore_deform.h states the contract these lines implement).  Pure
// float32 functions with no memory of their own beyond the pointers they are handed, so that k_deform_pose in hr_deform.hip and the CPU
// test (tests/host/deform_cpu.cpp, against heatray_amd/deform.py) compile the same lines.  v3, msValid and msNormalize come from hr_mesh.h.
#pragma once
#include "hr_mesh.h"

namespace hr {

static constexpr float kDfLargest = 3.0e37f; // "finite": |x| <= this (hr_geom_add's rule for a position)

// what a pose reads beside the rest pose; PF / PU: pointers to float / uint32_t words (the kernel's are global-address-space ones)
template <class PF, class PU> struct DfRig {
    PF dP, dN;      // nMorph x V x 3 (dN null: normals are not morphed)
    PU joints;      // V x 4
    PF weights;     // V x 4
    PF morphW;      // nMorph
    PF mats;        // nJoints x 16, column-major
    uint32_t V;
    int32_t nMorph, nJoints;
};

template <class PF> HRN v3 dfLoad3(PF a, size_t i) { return v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }

template <class PF> HRN v3 dfPoint(PF M, v3 p)
{
    return v3(((M[0] * p.x + M[4] * p.y) + M[8] * p.z) + M[12], ((M[1] * p.x + M[5] * p.y) + M[9] * p.z) + M[13], ((M[2] * p.x + M[6] * p.y) + M[10] * p.z) + M[14]);
}
template <class PF> HRN v3 dfDir(PF M, v3 d)
{
    return v3((M[0] * d.x + M[4] * d.y) + M[8] * d.z, (M[1] * d.x + M[5] * d.y) + M[9] * d.z, (M[2] * d.x + M[6] * d.y) + M[10] * d.z);
}

HRN bool dfFinite(v3 p) { return abs_(p.x) <= kDfLargest && abs_(p.y) <= kDfLargest && abs_(p.z) <= kDfLargest; } // (a NaN compares false)

// a posed direction normalised; false where its length is not valid
HRN bool dfDirection(v3 &d)
{
    if (!msValid(dot(d, d))) return false;
    d = msNormalize(d);
    return true;
}

// x + the K deltas of vertex v, each times its morph weight, one after the other
template <class PF, class PU> HRN v3 dfMorph(const DfRig<PF, PU> &r, PF deltas, uint32_t v, v3 x)
{
    for (int k = 0; k < r.nMorph; ++k) x = x + dfLoad3(deltas, (size_t)k * r.V + v) * r.morphW[k];
    return x;
}

// the weighted sum over vertex v's four influences of the joint's matrix applied to x, as a point or as a direction; x itself without joints
template <bool POINT, class PF, class PU> HRN v3 dfSkin(const DfRig<PF, PU> &r, uint32_t v, v3 x)
{
    if (r.nJoints <= 0) return x;
    v3 X(0.0f);
    for (int i = 0; i < 4; ++i) {
        const float w = r.weights[4 * (size_t)v + i];
        if (w == 0.0f) continue;
        const PF M = r.mats + 16 * (size_t)r.joints[4 * (size_t)v + i];
        X = X + (POINT ? dfPoint(M, x) : dfDir(M, x)) * w;
    }
    return X;
}

// Vertex v, one output at a time: the four are independent sums, so a kernel poses, finishes and stores one before it starts the next and
// never holds more than one rest value, one sum and one matrix in registers.  `keep`: the result is not usable (the position is not
// finite, the direction's length is not valid) and the rest value stays.  What is WRITTEN is the caller's: the normal only with dN or
// joints, tangent and bitangent only with joints on a mesh that has both.
template <class PF, class PU> HRN v3 dfPosePosition(const DfRig<PF, PU> &r, uint32_t v, v3 rest, bool &keep)
{
    const v3 p = dfSkin<true>(r, v, dfMorph(r, r.dP, v, rest));
    keep = !dfFinite(p);
    return keep ? rest : p;
}
template <class PF, class PU> HRN v3 dfPoseNormal(const DfRig<PF, PU> &r, uint32_t v, v3 rest, bool &keep)
{
    v3 n = dfSkin<false>(r, v, r.dN ? dfMorph(r, r.dN, v, rest) : rest);
    keep = !dfDirection(n);
    return keep ? rest : n;
}
template <class PF, class PU> HRN v3 dfPoseFrame(const DfRig<PF, PU> &r, uint32_t v, v3 rest, bool &keep) // a tangent or a bitangent
{
    v3 t = dfSkin<false>(r, v, rest);
    keep = !dfDirection(t);
    return keep ? rest : t;
}

} // namespace hr
