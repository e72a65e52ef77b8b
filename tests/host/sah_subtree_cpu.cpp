// heatray_amd/csrc/hr_sah_subtree.h on the CPU (tests/test_sah_subtree.py builds this with -fsanitize=address,undefined and runs it): the
// phases of k_sah_subtrees driven lane by lane, as the wave runs them, on the bottom subtrees of radix trees built here the way k_karras
// builds them.  Without arguments: the self-test (about 10^4 subtrees of random scenes, then the hostile ones); prints "sah subtree cpu: ok"
// and returns 0 when every check holds.  With IN OUT: IN holds int32 count, then per subtree int32 m and m boxes of 6 floats (lo, hi);
// OUT gets, per subtree, m - 1 pairs of int32 (axis, k): the split of every node slot, for the numpy port of tools/tree_proto.py's
// sah_sweep in the same test file.
#include "hr_sah_subtree.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond) && ++failures <= 20) printf("line %d: %s\n", __LINE__, #cond);       \
    } while (0)

struct Box {
    float lo[3], hi[3];
};
struct RNode {
    int left, right, first, last;
};

// the wave: every phase for every lane, then the next (k_sah_subtrees); returns the levels (= depth), 0 when it gave up at maxDepth
static int build(SahSub &s, const Box *b, int m, int maxDepth)
{
    std::memset(&s, 0, sizeof(s));
    s.m = m;
    for (int l = 0; l < m; ++l)
        for (int q = 0; q < 3; ++q) s.lo[q][l] = b[l].lo[q], s.hi[q][l] = b[l].hi[q];
    for (int l = 0; l < kSahMax; ++l) sahInit(s, l);
    int levels = 0;
    for (;;) {
        for (int l = 0; l < kSahMax; ++l) sahCandidate(s, l, levels & 1);
        bool more = false;
        for (int l = 0; l < kSahMax; ++l) more |= sahPartition(s, l, levels & 1, levels);
        ++levels;
        if (!more) break;
        if (levels >= maxDepth) return 0;
    }
    for (int lv = levels - 1; lv >= 0; --lv)
        for (int l = 0; l < kSahMax; ++l) sahEvaluate(s, l, lv);
    return levels;
}

// ---- a radix tree as k_karras makes it (hr_build.hip), on the host
static int delta(const std::vector<uint32_t> &keys, int i, int j)
{
    const int n = (int)keys.size();
    if (j < 0 || j >= n) return -1;
    if (keys[i] == keys[j]) return 32 + __builtin_clz((uint32_t)i ^ (uint32_t)j);
    return __builtin_clz(keys[i] ^ keys[j]);
}
static std::vector<RNode> karras(const std::vector<uint32_t> &keys)
{
    const int n = (int)keys.size();
    std::vector<RNode> nodes(n - 1);
    for (int i = 0; i < n - 1; ++i) {
        const int d = (delta(keys, i, i + 1) - delta(keys, i, i - 1)) >= 0 ? 1 : -1;
        const int dmin = delta(keys, i, i - d);
        int lmax = 2;
        while (delta(keys, i, i + lmax * d) > dmin) lmax *= 2;
        int l = 0;
        for (int t = lmax / 2; t >= 1; t /= 2)
            if (delta(keys, i, i + (l + t) * d) > dmin) l += t;
        const int j = i + l * d, dnode = delta(keys, i, j);
        int s = 0, t = l;
        do {
            t = (t + 1) >> 1;
            if (delta(keys, i, i + (s + t) * d) > dnode) s += t;
        } while (t > 1);
        const int gamma = i + s * d + (d < 0 ? d : 0), lo = std::min(i, j), hi = std::max(i, j);
        nodes[i] = RNode{lo == gamma ? ~gamma : gamma, hi == gamma + 1 ? ~(gamma + 1) : gamma + 1, lo, hi};
    }
    return nodes;
}

struct Eval {
    SahCost cost;
    int depth;
    Box box;
};
template <class Children, class Leaf>
static Eval evaluate(int ref, const Children &children, const Leaf &leaf, std::vector<int> *leaves, std::vector<int> *inner)
{
    if (ref < 0) {
        if (leaves) leaves->push_back(~ref);
        return Eval{{0, 0, 0, 0}, 0, leaf(~ref)};
    }
    if (inner) inner->push_back(ref);
    int l, r;
    children(ref, l, r);
    const Eval a = evaluate(l, children, leaf, leaves, inner), b = evaluate(r, children, leaf, leaves, inner);
    Eval e;
    for (int q = 0; q < 3; ++q) e.box.lo[q] = sahMin(a.box.lo[q], b.box.lo[q]), e.box.hi[q] = sahMax(a.box.hi[q], b.box.hi[q]);
    e.cost = sahCollapseCost(a.cost, b.cost, sahArea(e.box.lo, e.box.hi));
    e.depth = 1 + std::max(a.depth, b.depth);
    return e;
}

static uint32_t rngState = 12345u;
static uint32_t rnd() { return rngState = rngState * 1664525u + 1013904223u; }
static float uni() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }

static uint32_t expand10(uint32_t v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu, v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u, v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

static long subtreesSeen = 0, subtreesKept = 0, sizeSeen[kSahMax + 1];

// every bottom subtree (3..T leaves under a node of more) of the radix tree over `boxes`, as k_sah_find lists them
static void runScene(std::vector<Box> boxes, int T)
{
    const int n = (int)boxes.size();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const Box &b : boxes)
        for (int q = 0; q < 3; ++q) lo[q] = std::min(lo[q], b.lo[q]), hi[q] = std::max(hi[q], b.hi[q]);
    std::vector<std::pair<uint32_t, int>> order(n);
    for (int i = 0; i < n; ++i) {
        uint32_t key = 0;
        for (int q = 0; q < 3; ++q) {
            const float ext = hi[q] - lo[q], c = (boxes[i].lo[q] + boxes[i].hi[q]) * 0.5f;
            const float f = ext > 0.0f ? (c - lo[q]) / ext : 0.0f;
            key |= expand10((uint32_t)std::min(std::max(f * 1024.0f, 0.0f), 1023.0f)) << (2 - q);
        }
        order[i] = {key, i};
    }
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint32_t, int> &a, const std::pair<uint32_t, int> &b) { return a.first < b.first; });
    std::vector<uint32_t> keys(n);
    std::vector<Box> sorted(n);
    for (int i = 0; i < n; ++i) keys[i] = order[i].first, sorted[i] = boxes[order[i].second];
    const std::vector<RNode> nodes = karras(keys);
    auto radixChildren = [&](int ref, int &l, int &r) { l = nodes[ref].left, r = nodes[ref].right; };
    auto radixLeaf = [&](int i) { return sorted[i]; };
    for (int p = 0; p < n - 1; ++p) {
        if (nodes[p].last - nodes[p].first + 1 <= T) continue;
        for (int side = 0; side < 2; ++side) {
            const int ch = side ? nodes[p].right : nodes[p].left;
            if (ch < 0) continue;
            const int first = nodes[ch].first, last = nodes[ch].last, m = last - first + 1;
            if (m > T || m < 3) continue;
            ++subtreesSeen, ++sizeSeen[m];
            std::vector<int> rLeaves, rInner;
            const Eval radix = evaluate(ch, radixChildren, radixLeaf, &rLeaves, &rInner);
            // the slots: the radix subtree's inner nodes are exactly base .. base + m - 2
            const int base = sahOwnedBase(first, last, ch);
            std::sort(rInner.begin(), rInner.end());
            CHECK((int)rInner.size() == m - 1 && rInner.front() == base && rInner.back() == base + m - 2 && base >= 0 && base + m - 2 <= n - 2);
            CHECK(ch == first || ch == last);
            static SahSub s, again;
            const int levels = build(s, &sorted[first], m, radix.depth);
            const int levels2 = build(again, &sorted[first], m, radix.depth);
            CHECK(levels == levels2 && std::memcmp(&s, &again, sizeof(s)) == 0); // the same bytes
            if (levels == 0) continue; // gave up: deeper than the radix subtree, which stays
            // a binary tree over exactly the given leaves, each once, in m - 1 slots 0 .. m - 2, each once
            std::vector<int> leaves, inner;
            bool inRange = true;
            for (int t = 0; t < m - 1; ++t) {
                for (const int ref : {s.left[t], s.right[t]}) inRange = inRange && (ref < 0 ? ~ref < m : (ref > t && ref < m - 1));
                inRange = inRange && s.level[t] >= 0 && s.level[t] < levels;
            }
            CHECK(inRange);
            if (!inRange) continue;
            auto newChildren = [&](int ref, int &l, int &r) { l = s.left[ref], r = s.right[ref]; };
            auto newLeaf = [&](int i) { return sorted[first + i]; };
            const Eval sweep = evaluate(0, newChildren, newLeaf, &leaves, &inner);
            std::sort(leaves.begin(), leaves.end()), std::sort(inner.begin(), inner.end());
            bool all = (int)leaves.size() == m && (int)inner.size() == m - 1;
            for (int t = 0; all && t < m; ++t) all = leaves[t] == t;
            for (int t = 0; all && t < m - 1; ++t) all = inner[t] == t;
            CHECK(all);
            // the phases' own evaluation is the tree's
            CHECK(sweep.depth == levels && std::memcmp(&sweep.cost, &s.cost[0], sizeof(SahCost)) == 0);
            for (int q = 0; q < 3; ++q) CHECK(sweep.box.lo[q] == s.nlo[q][0] && sweep.box.hi[q] == s.nhi[q][0] && sweep.box.lo[q] == radix.box.lo[q] && sweep.box.hi[q] == radix.box.hi[q]);
            // the kept version is never dearer and never deeper than the radix version
            const bool keep = sahKeep(s.cost[0].c1, levels, radix.cost.c1, radix.depth);
            const float keptC1 = keep ? sweep.cost.c1 : radix.cost.c1;
            const int keptDepth = keep ? sweep.depth : radix.depth;
            CHECK(keptC1 <= radix.cost.c1 && keptDepth <= radix.depth);
            CHECK(!keep || sweep.cost.c1 < radix.cost.c1);
            subtreesKept += keep ? 1 : 0;
        }
    }
}

enum Kind { kRandom, kSameCentroid, kCoincident, kPoints, kHuge };
static void cluster(std::vector<Box> &out, int count, Kind kind, float origin, float scale)
{
    const float centre[3] = {uni(), uni(), uni()};
    for (int i = 0; i < count; ++i) {
        Box b;
        for (int q = 0; q < 3; ++q) {
            float c = uni(), e = 0.02f + 0.1f * uni() * uni();
            if (kind == kSameCentroid || kind == kCoincident) c = centre[q];
            if (kind == kCoincident) e = 0.05f;
            if (kind == kPoints) e = 0.0f;
            b.lo[q] = (origin + 0.3f * (c - e)) * scale, b.hi[q] = (origin + 0.3f * (c + e)) * scale;
            if (kind == kSameCentroid) b.lo[q] = (origin + 0.125f - e) * scale, b.hi[q] = (origin + 0.125f + e) * scale; // (exactly symmetric: equal centroids)
        }
        out.push_back(b);
    }
}

static int selfTest()
{
    // random scenes of 65 .. 400 boxes of mixed sizes: about 10^4 bottom subtrees
    while (subtreesSeen < 10000) {
        const int n = 65 + (int)(rnd() % 336u);
        std::vector<Box> boxes;
        cluster(boxes, n, kRandom, 0.0f, 2.5f);
        runScene(boxes, (rnd() & 0x300u) ? 3 + (int)((rnd() >> 8) % 62u) : 64); // (T = 64 for a quarter of them)
    }
    const long randomSeen = subtreesSeen;
    // the hostile ones: a cluster of each kind and of sizes 3, 4, 63, 64 in one corner (centroids below 0.3), 64 boxes in the opposite corner
    // (above 0.7): the root's split separates them whatever the scene's bounds, and each cluster is one bottom subtree of exactly its size
    for (const Kind kind : {kRandom, kSameCentroid, kCoincident, kPoints, kHuge})
        for (const int size : {3, 4, 5, 17, 63, 64})
            for (const Kind other : {kRandom, kCoincident}) {
                const long before = sizeSeen[size];
                std::vector<Box> boxes;
                const float scale = kind == kHuge ? 1e30f : 1.0f;
                cluster(boxes, size, kind == kHuge ? kRandom : kind, 0.0f, scale);
                cluster(boxes, 64, other, 0.7f, scale);
                runScene(boxes, 64);
                if (!(sizeSeen[size] > before)) printf("kind %d size %d other %d\n", (int)kind, size, (int)other);
                CHECK(sizeSeen[size] > before);
            }
    for (const int size : {3, 4, 63, 64}) CHECK(sizeSeen[size] > 0);
    CHECK(subtreesKept > randomSeen / 4); // (the sweep wins most of the time on random boxes: the builder does something)
    printf("%ld subtrees, %ld kept\n", subtreesSeen, subtreesKept);
    return failures;
}

int main(int argc, char **argv)
{
    if (argc == 3) {
        FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
        int32_t count = 0;
        if (!f || !g || fread(&count, 4, 1, f) != 1) return 2;
        for (int32_t i = 0; i < count; ++i) {
            int32_t m = 0;
            if (fread(&m, 4, 1, f) != 1 || m < 2 || m > kSahMax) return 2;
            std::vector<Box> b(m);
            if (fread(b.data(), sizeof(Box), m, f) != (size_t)m) return 2;
            static SahSub s;
            if (build(s, b.data(), m, kSahMax) == 0) return 3;
            for (int t = 0; t < m - 1; ++t) {
                const int32_t pair[2] = {s.splitAxis[t], s.splitK[t]};
                fwrite(pair, 4, 2, g);
            }
        }
        fclose(f), fclose(g);
    } else if (selfTest())
        return printf("sah subtree cpu: %d checks failed\n", failures), 1;
    printf("sah subtree cpu: ok\n");
    return 0;
}
