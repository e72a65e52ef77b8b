// hr_packet_interval.h — the arithmetic of the camera-ray packet's INTERVAL box test (DESIGN.md §2 "Camera-ray packets: one interval
// box test per node").  Pure float32 functions, no memory of their own, compiled by the packet kernel (hr_raygen.hip: packetTraverseInterval)
// and by the CPU test (tests/host/packet_interval_cpu.cpp) from the same lines.
//
// The packet kernel enters a child of a node when ANY of its 64 rays' own slab tests enters it.  Each of those tests computes, per axis
// and plane byte q of the child,
//     t = fma(q, bx, ax)        bx = 2^e * id        ax = fma(a, id, -(o * id))        id = safeInv(d)
// (a: the node's origin, 2^e: its scale, o / d: the ray's), takes tn = max(tx, ty, tz, tmin) over the three entry planes and
// tf = min(tx, ty, tz, tlim) over the three exit planes and enters when tn <= tf.  The hit is defined by the triangle test alone
// (hr_trace.h), so the packet may enter MORE children than that without changing a bit of the result — never fewer.  What follows
// computes, ONCE for the packet, a value L <= every ray's t of an entry plane and a value U >= every ray's t of an exit plane, from the
// packet's bounds: per axis [idLo, idHi] of id (one sign), [oLo, oHi] of the origin.  (The kernel gives only packets with ONE origin to
// these lines, oLo = oHi: a box over origin and direction is far looser than the rays of a lens, DESIGN §2.  Origin intervals are
// exercised by the CPU test alone.)  max(L's, tmin) <= min(U's, max tlim) is then
// implied by any ray's tn <= tf.
//
// THE BOUND (way (b) of the two the issue names: the tight form with an error term — it does not widen when the scene lies far from
// the world's origin, as bounding a * id and o * id separately would).  In real arithmetic a ray's plane distance is
//     t* = (a + q S - o) id,        S = 2^e,
// bilinear in (o, id): over the box [oLo, oHi] x [idLo, idHi] it is smallest and largest at a corner.  With one sign of id the corner is
// known from the sign of p = a + q S - o alone:  min t* = pe * (pe >= 0 ? idLo : idHi) with pe = (id > 0 ? p(oHi) : p(oLo)), and
// max t* = pe * (pe >= 0 ? idHi : idLo) with pe = (id > 0 ? p(oLo) : p(oHi)).   (pkiLane picks o and the two ids once per packet.)
//
// THE ERROR TERM.  u = 2^-24, M = |a| + max|o| + 255 S, I = max|id|; every operation rounds to nearest, no overflow (guarded below):
//   the ray's own value   oi = o id (1+e1), ax = (a id - oi)(1+e2), t = (q bx + ax)(1+e3), bx exact (a power of two times id):
//                         |t - t*| <= u|o|I + u(|a| + |o|)I(1+u) + u(255 S + |a| + |o|)I(1+u)^2            <= 2 u M I (1+3u)
//   the corner here       c = a - o (1+e4), p = (q S + c)(1+e5): |p - p*| <= 2 u M (1+u);  r = p idk (1+e6):
//                         |r - p* idk| <= 2 u M I (1+u) + u |p| I                                          <= 3 u M I (1+2u)
//                         and where p and p* differ in sign (so both are <= 2 u M (1+u) in size) the OTHER id was the right one:
//                         both products are then at most 2 u M I (1+2u) in size                            <= 4 u M I (1+2u)
//   the last step         r -+ E rounds by at most u (|r| + E)                                             <= 1 u M I (1+..)
// together 7 u M I (1 + 4u).  E = 8 u (|a| + max|o| + 256 S) I, computed in floats (three roundings: (1 - 4u) of its real value at
// worst), covers that: 8 (1 - 4u) > 7 (1 + 4u), and 256 S for 255 S.  (The bound is a worst case: the CPU fuzz, which aims rays at the
// children's planes, edges and corners, finds its first violations with the factor at 1, none at 2.)  Results in the subnormal range are rounded by at most 2^-150
// absolutely instead of relatively (a handful of operations, one of them scaled by q <= 255; p itself is exact there: q S + c is a
// multiple of 2^-149): kPkiAbs = 1e-36 covers them.
//
// OVERFLOW AND NaN.  E <= kPkiMax means M I < 4.2e36: every intermediate above, the rays' own included, is finite and the bounds
// hold.  Otherwise (a scale exponent at the top of the range, a direction at the safeInv clamp against a distant node, a NaN
// anywhere) the plane's bound is -inf (entry) / +inf (exit): the axis constrains nothing, which is a superset of whatever the rays' own tests —
// whose max / min drop NaNs — make of it.
#pragma once
#include <stdint.h>

#ifdef HRD
#define HRP HRD
#else
#define HRP inline
#endif

namespace hr {

static const float kPkiClamp = 1e-20f;               // safeInv's limit (hr_trace.h): a component below it is clamped there
#ifndef HR_PKI_ERR_ULPS
// The constant rests on the derivation above, NOT on the fuzz: tests/test_packet_interval_ref.py builds the fuzz once more with the term
// at 1 u and 0.5 u and sees it fail, but finds nothing from 2 u up — a value between 2 and 7 would pass the tests and be wrong.
#define HR_PKI_ERR_ULPS 8.0f
#endif
static const float kPkiErr = HR_PKI_ERR_ULPS * 5.9604644775390625e-8f; // 8 u
static const float kPkiAbs = 1e-36f;
static const float kPkiMax = 4e30f;

// One axis of the packet's bounds, and what it says about the step the packet may take
struct PkiAxis {
    float idLo, idHi, oLo, oHi;
};
// uniform sign of 1 / d over the packet's rays (and nothing clamped, nothing that is not a finite number): the interval step applies
HRP bool pkiAxisUniform(const PkiAxis &b, bool anyClamped)
{
    const bool finite = __builtin_fabsf(b.idLo) < __builtin_inff() && __builtin_fabsf(b.idHi) < __builtin_inff() && __builtin_fabsf(b.oLo) < __builtin_inff() &&
                        __builtin_fabsf(b.oHi) < __builtin_inff();
    return finite && !anyClamped && (b.idLo > 0.0f || b.idHi < 0.0f);
}
HRP bool pkiClamped(float d) { return __builtin_fabsf(d) < kPkiClamp; }

// What one (axis, entry / exit) role keeps for the whole traversal.  An exit role works with the NEGATED distance (its ids carry the
// sign), so that both kinds of role fold the same way: max over the axes, the error term subtracted.
struct PkiLane {
    float oSel;  // the origin bound whose corner this role needs
    float idA;   // the id to multiply by when p >= 0 (negated in an exit role) ...
    float idB;   // ... and when p < 0
    float oAbs;  // max |o|
    float idErr; // 8 u max|id|
    uint32_t hi; // 1: this role reads the child's UPPER plane byte of the axis (exit plane of id > 0, entry plane of id < 0)
};
HRP PkiLane pkiLane(const PkiAxis &b, bool exitPlane)
{
    const bool neg = b.idHi < 0.0f;
    PkiLane L;
    // entry: min t*, exit: max t* (see above)
    L.oSel = (exitPlane != neg) ? b.oLo : b.oHi;
    L.idA = exitPlane ? -b.idHi : b.idLo;
    L.idB = exitPlane ? -b.idLo : b.idHi;
    L.oAbs = __builtin_fmaxf(__builtin_fabsf(b.oLo), __builtin_fabsf(b.oHi));
    L.idErr = kPkiErr * __builtin_fmaxf(__builtin_fabsf(b.idLo), __builtin_fabsf(b.idHi));
    L.hi = (exitPlane != neg) ? 1u : 0u;
    return L;
}

// The bound of one plane: q the child's plane byte (as a float), S = 2^e the node's scale and a its origin on this axis.
// Entry role: a value <= every ray's fma(q, bx, ax).  Exit role: a value <= MINUS every ray's fma(q, bx, ax).
// (p * -id is -(p * id) exactly, and x - E rounds as -(-x + E) does: the exit role's value is minus the upper bound r + E.)
HRP float pkiPlane(float q, float S, float a, const PkiLane &L)
{
    const float c = a - L.oSel;
    const float p = __builtin_fmaf(q, S, c);
    const float r = p * (p >= 0.0f ? L.idA : L.idB);
    const float M = __builtin_fmaf(256.0f, S, __builtin_fabsf(a) + L.oAbs);
    const float E = __builtin_fmaf(M, L.idErr, kPkiAbs);
    return (E <= kPkiMax) ? r - E : -__builtin_inff();
}

// The child's test from its six plane values, tmin and the packet's tlim (the kernel folds them across lanes — a quad of entry roles
// with tmin, a quad of exit roles with -tlim, max inside each, then entry <= -exit — here spelled out).  `lower` orders the children
// and is the packet's entry distance.
HRP bool pkiEnters(float lx, float ly, float lz, float tmin, float nux, float nuy, float nuz, float tlim, float &lower)
{
    lower = __builtin_fmaxf(__builtin_fmaxf(lx, ly), __builtin_fmaxf(lz, tmin));
    const float negUpper = __builtin_fmaxf(__builtin_fmaxf(nux, nuy), __builtin_fmaxf(nuz, -tlim));
    return lower <= -negUpper;
}

} // namespace hr
