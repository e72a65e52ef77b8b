// heatray_amd/csrc/hr_packet_interval.h on the CPU (tests/test_packet_interval_ref.py): a fuzz of (node, packet) pairs that holds the
// interval box test of the camera-ray packets against the per-ray test it replaces.  The per-ray lines below restate packetTraverse's
// (hr_raygen.hip) and safeInv / rayFrame (hr_trace.h), operation for operation; the interval side calls the header the kernel compiles.
// Input: uint32 seed, pairs.  Output: uint64 counters, see `Out`.
#include "hr_packet_interval.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hr;

struct Out {
    uint64_t pairs;        // (node, packet) pairs generated
    uint64_t stepPairs;    // ... whose packet takes the interval step
    uint64_t fallback;     // ... flagged for the per-ray step
    uint64_t violations;   // children some ray's own test entered and the interval test did not  (MUST be 0)
    uint64_t mixedMissed;  // packets with mixed signs, a clamped or a non-finite component that were NOT flagged  (MUST be 0)
    uint64_t anyEntered;   // children entered by some ray's own test, over the interval-step pairs
    uint64_t ivEntered;    // children entered by the interval test, same pairs
    uint64_t narrowAny;    // the same two over the narrow, well-conditioned pairs
    uint64_t narrowIv;
    uint64_t narrowPairs;
    uint64_t farAny;       // ... and over narrow pairs of a scene moved 10^3 .. 10^4 of its sizes away from the world's origin
    uint64_t farIv;
    uint64_t farPairs;
    uint64_t openPlanes;   // plane values that came out as -inf (the overflow guard)
    uint64_t diffOrigins;  // interval-step pairs whose rays do not share an origin
    uint64_t culledByTlim; // children the interval test left out although their boxes were entered up to tlim = inf
    uint64_t advPairs;     // interval-step pairs of the adversarial share: rays that graze one child's planes, edges and corners
    uint64_t advGrazes;    // ... child tests of that share where a ray's own entry and exit distances are within 4 ulps of each other
};

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33) ^ (uint32_t)(s >> 11);
    }
    double uni() { return (next() >> 8) * (1.0 / 16777216.0); }
    double range(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

static float safeInv(float d)
{
    const float lim = 1e-20f;
    if (__builtin_fabsf(d) < lim) d = (d < 0.0f) ? -lim : lim;
    return 1.0f / d;
}
static float asFloat(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

struct Node {
    float a[3];
    uint32_t e[3];
    uint8_t lo[3][4], hi[3][4];
};
struct Ray {
    float o[3], d[3], tlim;
};

// packetTraverse's child test for one ray
static bool rayEnters(const Node &n, const Ray &r, int c, float tmin, bool &graze)
{
    float tn = 0, tf = 0, tnk[3], tfk[3];
    for (int k = 0; k < 3; ++k) {
        const float id = safeInv(r.d[k]), oi = r.o[k] * id;
        const float b = asFloat(n.e[k] << 23) * id;
        const float a = __builtin_fmaf(n.a[k], id, -oi);
        const uint8_t nq = id < 0.0f ? n.hi[k][c] : n.lo[k][c], fq = id < 0.0f ? n.lo[k][c] : n.hi[k][c];
        tnk[k] = __builtin_fmaf((float)nq, b, a), tfk[k] = __builtin_fmaf((float)fq, b, a);
    }
    tn = __builtin_fmaxf(__builtin_fmaxf(tnk[0], tnk[1]), __builtin_fmaxf(tnk[2], tmin));
    tf = __builtin_fminf(__builtin_fminf(tfk[0], tfk[1]), __builtin_fminf(tfk[2], r.tlim));
    graze = graze || (tn <= tf ? std::nextafter(std::nextafter(std::nextafter(std::nextafter(tn, tf), tf), tf), tf) == tf
                               : std::nextafter(std::nextafter(std::nextafter(std::nextafter(tf, tn), tn), tn), tn) == tn);
    return tn <= tf;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hd[2];
    if (fread(hd, 4, 2, f) != 2) return 4;
    fclose(f);
    Rng g{hd[0] * 0x9E3779B97F4A7C15ull + 1u};
    Out out;
    memset(&out, 0, sizeof(out));
    const float inf = __builtin_inff();
    std::vector<Ray> rays(64);
    for (uint32_t it = 0; it < hd[1]; ++it) {
        // ---- the node: a box of about `size`, planes of 8 bits on a power-of-two scale per axis
        const int k2 = g.below(21) - 10;
        const double size = std::ldexp(1.0, k2);
        const bool extremeExp = g.below(20) == 0;
        const bool moved = g.below(3) == 0;
        double T[3] = {0, 0, 0};
        if (moved)
            for (int k = 0; k < 3; ++k) T[k] = (g.below(2) ? 1.0 : -1.0) * size * std::pow(10.0, g.range(3.0, 4.0));
        Node n;
        double centre[3];
        for (int k = 0; k < 3; ++k) {
            const double a = T[k] + size * g.range(-2.0, 2.0);
            n.a[k] = (float)a;
            int e = 127 + k2 - 8 + g.below(5) - 2;
            if (extremeExp && g.below(2)) e = g.below(2) ? 1 + g.below(3) : 252 + g.below(3);
            n.e[k] = (uint32_t)(e < 1 ? 1 : (e > 254 ? 254 : e));
            centre[k] = (double)n.a[k] + 128.0 * (double)asFloat(n.e[k] << 23);
            for (int c = 0; c < 4; ++c) {
                const int kind = g.below(10);
                int lo = g.below(256), hi = g.below(256);
                if (kind < 7 && lo > hi) { const int t = lo; lo = hi, hi = t; } // (kind 7, 8: as drawn, possibly inverted)
                if (kind == 9) hi = lo;                                          // degenerate: a flat box
                n.lo[k][c] = (uint8_t)lo, n.hi[k][c] = (uint8_t)hi;
            }
        }
        // ---- the packet: 1..64 rays from about `dist` away towards a point of the node's box, inside a cone of `foot` radians
        // ADVERSARIAL share (half): every ray is aimed at a point of ONE child's box whose coordinates lie exactly on the child's lower
        // or upper plane (so: on a face, an edge or a corner), the origin sometimes exactly in such a plane (a flat box seen edge-on
        // when lo = hi), and tlim is a ray's own plane distance of that child +- a few ulps: the cases where rounding decides tn <= tf
        const bool adv = g.below(2) == 0;
        const int advChild = g.below(4);
        const int nLive = adv && g.below(3) ? 1 + g.below(2) : 1 + g.below(64); // (few rays: tight bounds, the error term alone separates the two tests)
        const double dist = size * std::pow(10.0, g.range(-1.0, 4.0)); // (256 plane steps are about one `size`: up to 10^4 diagonals)
        const double foot = std::pow(10.0, g.range(-5.0, std::log10(0.3)));
        const bool shared = g.below(3) != 0;
        const double lens = shared ? 0.0 : dist * std::pow(10.0, g.range(-6.0, -2.0));
        const int tiny = g.below(8) == 0 ? g.below(3) : -1;   // one direction component close to or below the safeInv clamp
        const double tinyV = (g.below(2) ? 1.0 : -1.0) * std::pow(10.0, g.range(-26.0, -3.0));
        const bool tinyJitter = g.below(2) == 0;
        const int tlimKind = g.below(3); // 0: nothing hit yet, 1: every ray has a hit, 2: some have
        double dir[3], len = 0;
        for (int k = 0; k < 3; ++k) dir[k] = g.range(-1.0, 1.0), len += dir[k] * dir[k];
        len = std::sqrt(len) + 1e-30;
        double target[3], org[3];
        for (int k = 0; k < 3; ++k) {
            dir[k] /= len;
            target[k] = centre[k] + 128.0 * (double)asFloat(n.e[k] << 23) * g.range(-1.0, 1.0);
            org[k] = target[k] - dist * dir[k];
        }
        if (tiny >= 0) dir[tiny] = tinyV;
        if (adv && g.below(3) == 0) { // the origin exactly in one of the child's planes
            const int k = g.below(3);
            org[k] = (double)(float)((double)n.a[k] + (double)(g.below(2) ? n.hi[k][advChild] : n.lo[k][advChild]) * (double)asFloat(n.e[k] << 23));
        }
        for (int i = 0; i < nLive; ++i) {
            Ray &r = rays[i];
            double d[3], l2 = 0;
            for (int k = 0; k < 3; ++k) d[k] = dir[k] + foot * g.range(-1.0, 1.0), l2 += d[k] * d[k];
            if (tiny >= 0) d[tiny] = tinyJitter ? tinyV * g.range(-1.0, 2.0) : tinyV;
            if (adv) {
                for (int k = 0; k < 3; ++k) {
                    const double lo = n.lo[k][advChild], hi = n.hi[k][advChild];
                    const int m = g.below(8);
                    const double q = m < 3 ? lo : (m < 6 ? hi : (m == 6 ? g.range(lo, hi) : g.range(0.0, 255.0)));
                    d[k] = ((double)n.a[k] + q * (double)asFloat(n.e[k] << 23)) - org[k];
                }
                l2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
                if (!(l2 > 0.0)) d[0] = 1.0, l2 = 1.0;
            }
            l2 = std::sqrt(l2);
            for (int k = 0; k < 3; ++k) {
                r.d[k] = (float)(d[k] / l2);
                r.o[k] = (float)(org[k] + lens * g.range(-1.0, 1.0));
            }
            if (tiny >= 0) r.d[tiny] = (float)d[tiny];
            r.tlim = tlimKind == 0 || (tlimKind == 2 && g.below(2)) ? inf : (float)(dist * g.range(0.2, 1.8));
            if (adv && r.tlim < inf && g.below(4) != 0) { // the ray's own distance to one of the child's planes, a few ulps either way
                const int k = g.below(3);
                const float id = safeInv(r.d[k]), oi = r.o[k] * id;
                const float t = __builtin_fmaf((float)(g.below(2) ? n.hi[k][advChild] : n.lo[k][advChild]), asFloat(n.e[k] << 23) * id, __builtin_fmaf(n.a[k], id, -oi));
                if (t > 0.0f && t < inf) {
                    r.tlim = t;
                    for (int j = g.below(5) - 2; j != 0; j += j < 0 ? 1 : -1) r.tlim = std::nextafter(r.tlim, j < 0 ? 0.0f : inf);
                }
            }
        }
        const float tmin = g.below(4) == 0 ? 0.0f : (float)(size * 1e-5);
        ++out.pairs;
        // ---- the packet's bounds, as the kernel's wave reductions make them
        PkiAxis b[3];
        bool anyBad = false, mixedTruth = false;
        float tlimW = -inf;
        for (int k = 0; k < 3; ++k) {
            b[k] = PkiAxis{inf, -inf, inf, -inf};
            bool pos = false, neg = false;
            for (int i = 0; i < nLive; ++i) {
                const float id = safeInv(rays[i].d[k]);
                anyBad = anyBad || pkiClamped(rays[i].d[k]) || !(__builtin_fabsf(rays[i].d[k]) < inf) || !(__builtin_fabsf(rays[i].o[k]) < inf);
                b[k].idLo = __builtin_fminf(b[k].idLo, id), b[k].idHi = __builtin_fmaxf(b[k].idHi, id);
                b[k].oLo = __builtin_fminf(b[k].oLo, rays[i].o[k]), b[k].oHi = __builtin_fmaxf(b[k].oHi, rays[i].o[k]);
                pos = pos || id > 0.0f, neg = neg || id < 0.0f;
                if (__builtin_fabsf(rays[i].d[k]) < 1e-20f) mixedTruth = true; // (clamped: the same flag)
            }
            mixedTruth = mixedTruth || (pos && neg);
        }
        for (int i = 0; i < nLive; ++i) tlimW = __builtin_fmaxf(tlimW, rays[i].tlim);
        const bool step = pkiAxisUniform(b[0], anyBad) && pkiAxisUniform(b[1], anyBad) && pkiAxisUniform(b[2], anyBad);
        if (!step) {
            ++out.fallback;
            continue;
        }
        if (mixedTruth) ++out.mixedMissed;
        ++out.stepPairs;
        bool diff = false;
        for (int k = 0; k < 3; ++k) diff = diff || b[k].oLo != b[k].oHi;
        out.diffOrigins += diff ? 1 : 0;
        bool wellDir = true;
        for (int k = 0; k < 3; ++k) wellDir = wellDir && __builtin_fabsf(rays[0].d[k]) >= 0.05f;
        out.advPairs += adv ? 1 : 0;
        const bool narrow = !adv && foot <= 1e-3 && !diff && dist <= 100.0 * size && !extremeExp && tiny < 0 && wellDir && tlimKind == 0;
        PkiLane L[3][2];
        for (int k = 0; k < 3; ++k) L[k][0] = pkiLane(b[k], false), L[k][1] = pkiLane(b[k], true);
        for (int c = 0; c < 4; ++c) {
            float v[3][2];
            for (int k = 0; k < 3; ++k)
                for (int x = 0; x < 2; ++x) {
                    const uint8_t q = L[k][x].hi ? n.hi[k][c] : n.lo[k][c];
                    v[k][x] = pkiPlane((float)q, asFloat(n.e[k] << 23), n.a[k], L[k][x]);
                    out.openPlanes += (__builtin_fabsf(v[k][x]) == inf) ? 1 : 0;
                }
            float lower = 0, lowerOpen = 0;
            const bool iv = pkiEnters(v[0][0], v[1][0], v[2][0], tmin, v[0][1], v[1][1], v[2][1], tlimW, lower);
            const bool ivOpen = pkiEnters(v[0][0], v[1][0], v[2][0], tmin, v[0][1], v[1][1], v[2][1], inf, lowerOpen);
            out.culledByTlim += (ivOpen && !iv) ? 1 : 0;
            bool any = false, graze = false;
            for (int i = 0; i < nLive; ++i) any = any || rayEnters(n, rays[i], c, tmin, graze);
            out.advGrazes += (adv && graze) ? 1 : 0;
            if (any && !iv) ++out.violations;
            out.anyEntered += any ? 1 : 0, out.ivEntered += iv ? 1 : 0;
            if (narrow && !moved) out.narrowAny += any ? 1 : 0, out.narrowIv += iv ? 1 : 0;
            if (narrow && moved) out.farAny += any ? 1 : 0, out.farIv += iv ? 1 : 0;
        }
        if (narrow && !moved) ++out.narrowPairs;
        if (narrow && moved) ++out.farPairs;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(&out, sizeof(out), 1, f) != 1) return 6;
    fclose(f);
    printf("packet interval cpu: ok\n");
    return 0;
}
