// hr_mesh.h — the per-element arithmetic of mesh preparation (include/hrcore_mesh.h states the contract these lines implement).  Pure
// float32 functions with no memory of their own, so that the kernels in hr_mesh.hip and the CPU test (tests/host/mesh_cpu.cpp, against
// heatray_amd/meshprep.py) compile the same lines.  HRN and the host's sqrt_ / abs_ come from hr_denoise.h.
#pragma once
#include "hr_denoise.h"

#ifndef HRD
// The host build has no hr_math.h (it needs the HIP runtime): what is used below, in the same lines.
namespace hr {
struct v3 {
    float x, y, z;
    v3() {}
    v3(float a) : x(a), y(a), z(a) {}
    v3(float a, float b, float c) : x(a), y(b), z(c) {}
};
inline v3 operator+(v3 a, v3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline v3 operator-(v3 a, v3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline v3 operator*(v3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
inline v3 operator-(v3 a) { return v3(-a.x, -a.y, -a.z); }
inline float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline v3 cross(v3 a, v3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline float atan_(float xx)
{
    float x = abs_(xx);
    float y;
    if (x > 2.414213562373095f) {
        y = 1.5707963267948966192f;
        x = -(1.0f / x);
    } else if (x > 0.4142135623730950f) {
        y = 0.7853981633974483096f;
        x = (x - 1.0f) / (x + 1.0f);
    } else {
        y = 0.0f;
    }
    float z = x * x;
    y = y + ((((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z * x + x);
    return (xx < 0.0f) ? -y : y;
}
inline float atan2_(float y, float x)
{
    const float PIF = 3.14159265358979323846f;
    const float PIO2F = 1.5707963267948966192f;
    if (x == 0.0f) {
        if (y > 0.0f) return PIO2F;
        if (y < 0.0f) return -PIO2F;
        return 0.0f;
    }
    if (y == 0.0f) return (x < 0.0f) ? PIF : 0.0f;
    float w = 0.0f;
    if (x < 0.0f) w = (y < 0.0f) ? -PIF : PIF;
    return w + atan_(y / x);
}
} // namespace hr
#endif

namespace hr {

enum { MS_WEIGHT_ANGLE = 0, MS_WEIGHT_AREA = 1, MS_WEIGHT_UNIFORM = 2 };
// a triangle's flags: it contributes normal terms; it contributes tangent terms (never without MS_FACE)
enum { MS_FACE = 1, MS_UV = 2 };
// what became of a vertex's normal
enum { MS_NORMAL = 0, MS_CANCELLED = 1, MS_UNREFERENCED = 2 };

static constexpr uint32_t kMsNoCorner = 0xFFFFFFFFu; // "no non-degenerate corner"

HRN bool msValid(float l2) { return l2 > 0.0f && l2 < __builtin_inff(); }
HRN v3 msNormalize(v3 v) { return v * (1.0f / sqrt_(dot(v, v))); }

// the three vertex indices of triangle t of the list (include/hrcore_mesh.h, TRIANGLES)
template <class I> HRN void msTriangle(const I &idx, uint32_t t, bool strip, uint32_t id[3])
{
    if (strip) {
        id[0] = idx[(size_t)t], id[1] = idx[(size_t)t + 1], id[2] = idx[(size_t)t + 2];
        if (t & 1u) {
            const uint32_t s = id[0];
            id[0] = id[1], id[1] = s;
        }
    } else {
        id[0] = idx[3 * (size_t)t], id[1] = idx[3 * (size_t)t + 1], id[2] = idx[3 * (size_t)t + 2];
    }
}

// FACE TERMS: false for a DEGENERATE triangle; else u and the three corner weights
HRN bool msFace(v3 p0, v3 p1, v3 p2, int weight, v3 &e1, v3 &e2, v3 &u, float w[3])
{
    e1 = p1 - p0, e2 = p2 - p0;
    const v3 fn = cross(e1, e2);
    const float l2 = dot(fn, fn);
    u = v3(0.0f), w[0] = w[1] = w[2] = 0.0f;
    if (!msValid(l2)) return false;
    const float len = sqrt_(l2);
    u = fn * (1.0f / len);
    if (weight == MS_WEIGHT_ANGLE) {
        w[0] = atan2_(len, dot(e1, e2));
        w[1] = atan2_(len, dot(p2 - p1, p0 - p1));
        w[2] = atan2_(len, dot(p0 - p2, p1 - p2));
    } else {
        w[0] = w[1] = w[2] = weight == MS_WEIGHT_AREA ? len : 1.0f;
    }
    return true;
}

// the unit normal alone (the CANCELLED fallback recomputes it from the corner's triangle); the triangle is not DEGENERATE
HRN v3 msFaceUnit(v3 p0, v3 p1, v3 p2)
{
    const v3 fn = cross(p1 - p0, p2 - p0);
    return fn * (1.0f / sqrt_(dot(fn, fn)));
}

// TANGENTS of a non-degenerate triangle: false for a DEGENERATE-UV one; else the unit T and B
HRN bool msFaceTangents(v3 e1, v3 e2, float u0x, float u0y, float u1x, float u1y, float u2x, float u2y, v3 &Tn, v3 &Bn)
{
    const float d1x = u1x - u0x, d1y = u1y - u0y, d2x = u2x - u0x, d2y = u2y - u0y;
    const float det = d1x * d2y - d2x * d1y;
    v3 T = e1 * d2y - e2 * d1y, B = e2 * d1x - e1 * d2x;
    if (det < 0.0f) T = -T, B = -B;
    Tn = v3(0.0f), Bn = v3(0.0f);
    const float t2 = dot(T, T), b2 = dot(B, B);
    if (det == 0.0f || !(abs_(det) < __builtin_inff()) || !msValid(t2) || !msValid(b2)) return false;
    Tn = msNormalize(T), Bn = msNormalize(B);
    return true;
}

// NORMAL of a group from its sum G; `first` = the lowest-index non-degenerate corner of the group (kMsNoCorner: none), uFirst its
// triangle's u (read only when the sum is not valid and there is such a corner)
HRN int msFinishNormal(v3 G, uint32_t first, v3 uFirst, v3 &N)
{
    if (msValid(dot(G, G))) {
        N = msNormalize(G);
        return MS_NORMAL;
    }
    if (first == kMsNoCorner) {
        N = v3(0.0f);
        return MS_UNREFERENCED;
    }
    N = uFirst;
    return MS_CANCELLED;
}

// the caller's normal as the tangents' N: false (N = 0 0 0) when it cannot be normalised
HRN bool msGivenNormal(v3 n, v3 &N)
{
    N = v3(0.0f);
    if (!msValid(dot(n, n))) return false;
    N = msNormalize(n);
    return true;
}

// TANGENTS, finish: haveN false means N = 0 0 0.  Returns whether the tangent is the fallback.
HRN bool msFinishTangent(bool haveN, v3 N, v3 Ta, v3 Ba, v3 &tangent, v3 &bitangent)
{
    tangent = v3(0.0f), bitangent = v3(0.0f);
    if (!haveN) return false;
    const v3 t = Ta - N * dot(N, Ta);
    const bool own = msValid(dot(t, t));
    if (own) {
        tangent = msNormalize(t);
    } else {
        const float ax = abs_(N.x), ay = abs_(N.y), az = abs_(N.z);
        const v3 a = (ax <= ay && ax <= az) ? v3(1.0f, 0.0f, 0.0f) : (ay <= az ? v3(0.0f, 1.0f, 0.0f) : v3(0.0f, 0.0f, 1.0f));
        tangent = msNormalize(a - N * dot(N, a));
    }
    const v3 c = cross(N, tangent);
    bitangent = dot(c, Ba) < 0.0f ? -c : c;
    return !own;
}

} // namespace hr
