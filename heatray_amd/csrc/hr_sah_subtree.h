// hr_sah_subtree.h — the arithmetic of k_sah_subtrees (hr_build.hip): a bottom subtree of the radix tree (at most 64 triangles) rebuilt
// top-down by full-sweep SAH, one wave per subtree, lane = triangle.  Pure functions over one block of memory (SahSub: LDS on the
// device, a plain struct on the host), written as PHASES: every lane runs a phase, then all lanes meet (a barrier on the device, the end
// of the loop over lanes on the host), then the next phase.  A phase reads only what earlier phases or the lane itself wrote, so running the
// lanes one after another (tests/host/sah_subtree_cpu.cpp) gives the bytes the wave gives.
//
// The criterion is tools/tree_proto.py's sah_sweep: per range and axis the leaves ordered by centroid, cost(k) = A_L k + A_R (m - k) for
// the first k against the rest, the least over k and the three axes; ties go to the lower axis, then the lower k (argmin's first, the
// strict < between axes).  Equal centroids are ordered by the leaf's index: the order is total, so the same leaves always give the same
// tree.  Nothing is sorted: the candidate "the leaves up to and including leaf i in the order of axis a" is evaluated by lane i with one
// loop over the subtree's leaves (all lanes read the same leaf at the same time), and every range of a level is split in the same phase.
//
// Slots.  A range of c leaves owns c - 1 consecutive node slots starting at its `base`; its node is `base`, its first k leaves get
// base + 1 .. base + k - 1 and the rest base + k .. base + c - 2.  The root is slot 0 and every slot is used once: the m - 1 slots the radix
// subtree owned (sahOwnedBase) hold the new one.  The number of levels is the new tree's depth: the build gives up (keeps the radix
// subtree) once it exceeds the radix subtree's, which is what bounds the traversal stack.
#pragma once
#include <stdint.h>

#ifdef HRD
#define HRS HRD
#else
#define HRS inline
#endif

#ifdef __clang__
#define HRS_UNROLL _Pragma("unroll") // (the boxes of phase A are indexed by loop counters: unrolled they are registers)
#else
#define HRS_UNROLL
#endif

static const int kSahMax = 64; // leaves of a subtree: one wave

struct SahCost {
    float c1, c2, c3, c4; // k_refit_round's collapse costs (hr_build.hip)
};

struct SahSub {
    int m;                                // leaves
    float lo[3][kSahMax], hi[3][kSahMax]; // their boxes
    int base[2][kSahMax], cnt[2][kSahMax]; // per leaf, ping-pong by level: its range's node slot and leaf count (-1, 1: the leaf is placed)
    float candCost[kSahMax];              // each lane's best candidate of the level ...
    int candAxis[kSahMax], candK[kSahMax]; // ... (candK = 0: none)
    int left[kSahMax], right[kSahMax];    // the tree: >= 0 a slot, < 0 leaf ~index
    int level[kSahMax];                   // the level that made the slot
    int splitAxis[kSahMax], splitK[kSahMax]; // ... and its split: the first splitK leaves in the order of splitAxis go left
    float nlo[3][kSahMax], nhi[3][kSahMax]; // node boxes
    SahCost cost[kSahMax];
};

HRS float sahMin(float x, float y) { return (y < x) ? y : x; } // hr_math.h's fmin_ / fmax_
HRS float sahMax(float x, float y) { return (x < y) ? y : x; }
HRS float sahArea(const float lo[3], const float hi[3]) // boxArea
{
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx * dy + dy * dz + dz * dx;
}
// collapseCost of hr_build.hip on values: (C1..C4) of a binary node from its children's; a triangle child costs nothing
HRS SahCost sahCollapseCost(const SahCost &cl, const SahCost &cr, float area)
{
    const float h2 = cl.c1 + cr.c1;
    const float h3 = sahMin(cl.c1 + cr.c2, cl.c2 + cr.c1);
    const float h4 = sahMin(cl.c1 + cr.c3, sahMin(cl.c2 + cr.c2, cl.c3 + cr.c1));
    SahCost c;
    c.c1 = area + h4;
    c.c2 = sahMin(c.c1, h2), c.c3 = sahMin(c.c2, h3), c.c4 = sahMin(c.c3, h4);
    return c;
}

// The radix tree (k_karras) gives a node that covers sorted triangles first..last the index `first` when it is a right child (or the
// root) and `last` when it is a left child, and its inner descendants the other indices of first..last - 1 / first + 1..last.
HRS int sahOwnedBase(int first, int last, int rootIndex) { return rootIndex == last ? first + 1 : first; }

// leaf i comes before leaf j in the order of axis a, or is j (centroid, then index)
HRS bool sahNotAfter(float ci, int i, float cj, int j) { return ci < cj || (ci == cj && i <= j); }

// ---- phase 0 (after the lane has stored its box): everything is one range at slot 0
HRS void sahInit(SahSub &s, int lane)
{
    if (lane >= s.m) return;
    s.base[0][lane] = 0, s.cnt[0][lane] = s.m;
}

// ---- phase A of level `lv` (cur = lv & 1): the lane's best candidate over the three axes
HRS void sahCandidate(SahSub &s, int lane, int cur)
{
    if (lane >= s.m) return;
    s.candK[lane] = 0;
    const int c = s.cnt[cur][lane], b = s.base[cur][lane];
    if (c <= 1) return;
    float ci[3];
    HRS_UNROLL
    for (int a = 0; a < 3; ++a) ci[a] = (s.lo[a][lane] + s.hi[a][lane]) * 0.5f;
    const float inf = __builtin_inff();
    float llo[3][3], lhi[3][3], rlo[3][3], rhi[3][3]; // [axis of the order][coordinate]
    int k[3] = {0, 0, 0};
    HRS_UNROLL
    for (int a = 0; a < 3; ++a)
        HRS_UNROLL
        for (int q = 0; q < 3; ++q) llo[a][q] = rlo[a][q] = inf, lhi[a][q] = rhi[a][q] = -inf;
    for (int j = 0; j < s.m; ++j) {
        if (s.base[cur][j] != b) continue;
        float jl[3], jh[3];
        HRS_UNROLL
        for (int q = 0; q < 3; ++q) jl[q] = s.lo[q][j], jh[q] = s.hi[q][j];
        HRS_UNROLL
        for (int a = 0; a < 3; ++a) {
            const bool isLeft = sahNotAfter((jl[a] + jh[a]) * 0.5f, j, ci[a], lane);
            k[a] += isLeft ? 1 : 0;
            HRS_UNROLL
            for (int q = 0; q < 3; ++q) {
                if (isLeft)
                    llo[a][q] = sahMin(llo[a][q], jl[q]), lhi[a][q] = sahMax(lhi[a][q], jh[q]);
                else
                    rlo[a][q] = sahMin(rlo[a][q], jl[q]), rhi[a][q] = sahMax(rhi[a][q], jh[q]);
            }
        }
    }
    float best = 0.0f;
    int bestAxis = 0, bestK = 0;
    HRS_UNROLL
    for (int a = 0; a < 3; ++a) {
        if (k[a] >= c) continue; // the last leaf of the order: nothing on the right
        const float cost = sahArea(llo[a], lhi[a]) * (float)k[a] + sahArea(rlo[a], rhi[a]) * (float)(c - k[a]);
        if (bestK == 0 || cost < best) best = cost, bestAxis = a, bestK = k[a];
    }
    s.candCost[lane] = best, s.candAxis[lane] = bestAxis, s.candK[lane] = bestK;
}

// ---- phase B of level `lv`: the range's winner (cost, then axis, then k), the lane's side of it, the new node.
// Returns true while the lane's leaf is in a range of more than one leaf (another level is needed).
HRS bool sahPartition(SahSub &s, int lane, int cur, int lv)
{
    if (lane >= s.m) return false;
    const int c = s.cnt[cur][lane], b = s.base[cur][lane];
    if (c <= 1) {
        s.base[cur ^ 1][lane] = b, s.cnt[cur ^ 1][lane] = c;
        return false;
    }
    int w = -1;
    for (int j = 0; j < s.m; ++j) {
        if (s.base[cur][j] != b || s.candK[j] == 0) continue;
        if (w < 0 || s.candCost[j] < s.candCost[w] ||
            (s.candCost[j] == s.candCost[w] && (s.candAxis[j] < s.candAxis[w] || (s.candAxis[j] == s.candAxis[w] && s.candK[j] < s.candK[w]))))
            w = j;
    }
    // (w >= 0: in every axis all leaves of the range but the last of its order are candidates, and a range has at least two)
    const int a = s.candAxis[w], k = s.candK[w];
    const bool isLeft = sahNotAfter((s.lo[a][lane] + s.hi[a][lane]) * 0.5f, lane, (s.lo[a][w] + s.hi[a][w]) * 0.5f, w);
    const int nc = isLeft ? k : c - k, nb = nc == 1 ? -1 : (isLeft ? b + 1 : b + k); // (a placed leaf is in no range: no slot is -1)
    s.base[cur ^ 1][lane] = nb, s.cnt[cur ^ 1][lane] = nc;
    if (lane == w) { // (the winner is the last of the left side)
        s.level[b] = lv, s.splitAxis[b] = a, s.splitK[b] = k;
        s.left[b] = k == 1 ? ~lane : b + 1;
        if (c - k > 1) s.right[b] = b + k;
    } else if (!isLeft && nc == 1)
        s.right[b] = ~lane;
    return nc > 1;
}

// ---- phase C, for lv = levels - 1 down to 0: box and collapse costs of the slots made by level lv (lane = slot, < m - 1)
HRS void sahEvaluate(SahSub &s, int lane, int lv)
{
    if (lane >= s.m - 1 || s.level[lane] != lv) return;
    const int l = s.left[lane], r = s.right[lane];
    const SahCost zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int q = 0; q < 3; ++q) {
        s.nlo[q][lane] = sahMin(l < 0 ? s.lo[q][~l] : s.nlo[q][l], r < 0 ? s.lo[q][~r] : s.nlo[q][r]);
        s.nhi[q][lane] = sahMax(l < 0 ? s.hi[q][~l] : s.nhi[q][l], r < 0 ? s.hi[q][~r] : s.nhi[q][r]);
    }
    float blo[3], bhi[3];
    for (int q = 0; q < 3; ++q) blo[q] = s.nlo[q][lane], bhi[q] = s.nhi[q][lane];
    s.cost[lane] = sahCollapseCost(l < 0 ? zero : s.cost[l], r < 0 ? zero : s.cost[r], sahArea(blo, bhi));
}

// the sweep's subtree replaces the radix one only where it is cheaper by the measure the collapse minimises AND not deeper
HRS bool sahKeep(float sweepC1, int sweepDepth, float radixC1, int radixDepth) { return sweepC1 < radixC1 && sweepDepth <= radixDepth; }
