// hr_query.h — the per-ray arithmetic of ray queries (include/hrcore_query.h states the contract these lines implement): which rays are
// traced, the surface record of a closest hit, the camera ray of a pixel query.  Pure float32 functions with no memory of their own
// beyond the pointers they are handed; the kernels of hr_query.hip call them, heatray_amd/query.py restates them in numpy.  v3, msValid
// and msNormalize come from hr_mesh.h, dfPoint and dfDir (the contract's point and dir) from hr_deform.h.
#pragma once
#include "hr_deform.h"
#include "hr_types.h"
#include "../../include/hrcore_query.h"

namespace hr {

HRN bool qyFinite(float x) { return abs_(x) < __builtin_inff(); } // (a NaN compares false)

// Is the ray traced?  tmax = +inf where the caller gave none.
HRN bool qyRayValid(v3 o, v3 d, float tmax)
{
    const bool finite = qyFinite(o.x) && qyFinite(o.y) && qyFinite(o.z) && qyFinite(d.x) && qyFinite(d.y) && qyFinite(d.z);
    const bool zero = d.x == 0.0f && d.y == 0.0f && d.z == 0.0f;
    return finite && !zero && tmax > -__builtin_inff(); // (a NaN tmax compares false; +inf is "no limit")
}

HRN v3 qyUnitOrZero(v3 x) { return msValid(dot(x, x)) ? msNormalize(x) : v3(0.0f); }

// What a surface record holds beside the mesh's identity.  n9: the triangle's three world normals, uv6: its three uvs (TriAttr);
// e1, e2: the world-space edges k_assemble stored (Tri); ccw: the winding bit of the hit (HitRec::prim bit 31); triFlags: TF_*.
struct QySurface {
    v3 position, normal, geometric;
    float uv[2];
    uint32_t flags;
};
template <class PF> HRN QySurface qySurface(PF n9, PF uv6, uint32_t triFlags, v3 e1, v3 e2, v3 o, v3 d, float t, float u, float v, bool ccw)
{
    QySurface s;
    const float w = (1.0f - u) - v;
    s.position = o + d * t;
    const v3 N = (v3(n9[0], n9[1], n9[2]) * w + v3(n9[3], n9[4], n9[5]) * u) + v3(n9[6], n9[7], n9[8]) * v;
    s.normal = qyUnitOrZero(N);
    s.geometric = qyUnitOrZero(cross(e1, e2));
    const bool hasUv = (triFlags & TF_HAS_UV) != 0;
    s.uv[0] = hasUv ? (uv6[0] * w + uv6[2] * u) + uv6[4] * v : 0.0f;
    s.uv[1] = hasUv ? (uv6[1] * w + uv6[3] * u) + uv6[5] * v : 0.0f;
    const bool front = (triFlags & TF_FRONT_CW) ? !ccw : ccw; // rl_FrontFacing (hr_shade.h: Surface::frontFacing)
    s.flags = (front ? HR_QUERY_SF_FRONT : 0u) | (hasUv ? HR_QUERY_SF_HAS_UV : 0u) | ((triFlags & TF_NON_OCCLUDER) ? HR_QUERY_SF_NON_OCCLUDER : 0u);
    return s;
}

// The ray through the point (px, py) of a W x H frame from the centre of the lens: generatePrimary (hr_shade.h) without the jitter and
// with the aperture sample 0 0.
template <class PF> HRN void qyCameraRay(PF view, float fovTan, float aspect, float focus, float W, float H, float px, float py, v3 &o, v3 &d)
{
    const float u = px / W, v = py / H;
    const float cx = ((2.0f * u - 1.0f) * aspect) * fovTan;
    const float cy = ((1.0f - 2.0f * v) * fovTan) * -1.0f;
    const v3 c = msNormalize(v3(cx, cy, -1.0f));
    o = dfPoint(view, v3(0.0f));
    d = msNormalize(dfDir(view, focus * c));
}

} // namespace hr
