// Structural checks of a compressed 8-wide tree given as plain arrays (TEST INFRASTRUCTURE: used by
// tests/cpp/wide8_check.cpp on the tree it builds and by tests/cpp/wide_tree_check.cpp on arrays
// downloaded with pt_scene_download_wide; the product never uses it).  The record layout is the one
// host/pt_wide8.cpp documents.  Every check is exact: a plane decodes in fp64 as origin + q * 2^e
// without rounding (24 + 8 bits), and the boxes compared against are the primitives' exact fp32 boxes.
//
// What a tree that passes guarantees, whichever builder wrote it:
//   - the primitive records are a permutation of the scene's (every rank once, each record the
//     one of its object), and the leaf children's ranges [R[5] + offset, + count) tile [0, n): no
//     primitive is referenced twice, none is dropped;
//   - every child's decoded planes contain the exact box of every primitive below it with at least
//     the tree's smallest quantum 2^emin to spare on every side (emin = ceil(log2(ext)) -
//     kW8EminShift, clamped at -100; ext: the larger of the scene's extent and coordinates) -- the
//     outward margin the traversal's rounding bound needs (pt_device.hip wideHits);
//   - every encoding is in range: unary leaf counts, leaf offset + count <= 24, an internal child's
//     low meta bits equal to its slot, child bases below 2^24, exponent bytes <= 126 + 127;
//   - every reachable slot, and the end of every child block, lies within the reported slots, which
//     lie within the capacity and below 2^24; every reachable node is reached once;
//   - the reported depth is the deepest level the walk reaches (root = 1) and at most 24, the
//     deepest stack the kernels have (wideStackFor).
// A failed check prints "CHECK FAILED: <name> (<where>)" once per name, with the number of failures
// of that name in the summary line.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pt_wide8.hpp"

namespace widecheck {

struct Report {
    std::map<std::string, long> counts;
    long failures = 0;
    void check(bool ok, const char* name, long long where = -1, long long what = -1) {
        if (ok) return;
        failures++;
        if (counts[name]++ == 0) std::fprintf(stderr, "CHECK FAILED: %s (at %lld, %lld)\n", name, where, what);
    }
    void summary() const {
        for (const auto& c : counts) std::fprintf(stderr, "  %ld x %s\n", c.second, c.first.c_str());
    }
};

struct WideArrays {
    const uint32_t* nodes;      // nodeSlots x kW8NodeDwords dwords (what the array holds; reads stay inside it)
    int64_t nodeSlots;
    const uint32_t* prims;      // n x 12 dwords, the tree's leaf order, dword 3 = reference rank
    int64_t n;
    const uint32_t* leafPrims;  // n x 12 dwords, the LBVH's leaf order (pt::primRecord), or null: records not compared
    const float* leafBoxes;     // n x {min xyz, max xyz}, exact, LBVH leaf order
    const uint32_t* rank;       // LBVH leaf k -> reference rank
    int depth;                  // reported
    int64_t slots;              // reported
    int64_t capacity;           // node slots the builder may use
};

struct WalkResult {
    int64_t reached = 0;   // nodes
    int64_t leaves = 0;    // leaf children
    int depth = 0;         // deepest level, root = 1
    int emin = 0;
};

inline uint32_t metaOf(const uint32_t* R, int j) { return ((j < 4 ? R[6] : R[7]) >> (8 * (j & 3))) & 0xffu; }
inline bool isInternal(uint32_t meta) { return (meta & 0x18u) == 0x18u; }

// The smallest quantum's exponent, as both builders take it from the exact boxes
inline int eminOf(const float* boxes, int64_t n) {
    double ext = 0.0;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t k = 0; k < n; k++)
        for (int a = 0; a < 3; a++) {
            mn[a] = std::fmin(mn[a], (double)boxes[(size_t)k * 6 + a]);
            mx[a] = std::fmax(mx[a], (double)boxes[(size_t)k * 6 + 3 + a]);
        }
    for (int a = 0; a < 3; a++) ext = std::fmax(ext, std::fmax(std::fmax(std::fabs(mn[a]), std::fabs(mx[a])), mx[a] - mn[a]));
    return ext > 0.0 ? std::max(-100, (int)std::ceil(std::log2(ext)) - pt::kW8EminShift) : -100;
}

inline WalkResult checkWideTree(const WideArrays& A, Report& rep) {
    constexpr int D = pt::kW8NodeDwords;
    WalkResult res;
    const int64_t n = A.n;
    res.emin = eminOf(A.leafBoxes, n);
    const double minQuantum = std::ldexp(1.0, res.emin);
    // the records
    std::vector<int> seen((size_t)n, 0);
    std::vector<int64_t> kOfRank((size_t)n, -1);
    for (int64_t k = 0; k < n; k++) {
        const bool inRange = A.rank[k] < (uint32_t)n;
        rep.check(inRange && kOfRank[A.rank[k]] < 0, "reference ranks are a permutation", k);
        if (inRange) kOfRank[A.rank[k]] = k;
    }
    for (int64_t i = 0; i < n; i++) {
        const uint32_t* P = A.prims + (size_t)i * 12;
        const uint32_t rk = P[3];
        rep.check(rk < (uint32_t)n, "rank in range", i, rk);
        if (!(rk < (uint32_t)n)) continue;
        seen[rk]++;
        const int64_t k = kOfRank[rk];
        if (A.leafPrims && k >= 0) {
            const uint32_t* L = A.leafPrims + (size_t)k * 12;
            bool same = true;
            for (int d = 0; d < 12; d++) same = same && (d == 3 || P[d] == L[d]);
            rep.check(same, "primitive record is the one of its rank", i, rk);
        }
    }
    for (int64_t k = 0; k < n; k++) rep.check(seen[k] == 1, "every primitive exactly once", k, seen[k]);

    // the reported sizes
    rep.check(A.slots >= 1 && A.slots <= A.nodeSlots, "reported slots within the node array", A.slots, A.nodeSlots);
    rep.check(A.slots <= A.capacity, "reported slots within the capacity", A.slots, A.capacity);
    rep.check(A.slots < ((int64_t)1 << 24), "reported slots below 2^24", A.slots);
    rep.check(A.depth <= 24, "reported depth at most 24", A.depth);
    const int64_t bound = std::min(A.slots, A.nodeSlots);   // what the walk may read
    if (bound < 1) return res;

    auto prim = [&](int64_t i) -> int64_t {   // the LBVH leaf of wide-order primitive i, or -1
        if (i < 0 || i >= n) return -1;
        const uint32_t rk = A.prims[(size_t)i * 12 + 3];
        return rk < (uint32_t)n ? kOfRank[rk] : -1;
    };
    std::vector<int> visits((size_t)bound, 0);
    std::vector<int64_t> stamp((size_t)bound, -1);
    std::vector<std::pair<int64_t, int64_t>> ranges;   // leaf children: {first, count}
    struct Item { int64_t slot; int level; };
    std::vector<Item> todo{{0, 1}};
    visits[0] = 1;
    int64_t walkId = 0;
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        res.reached++;
        res.depth = std::max(res.depth, it.level);
        const int64_t s = it.slot;
        const uint32_t* R = A.nodes + (size_t)s * D;
        for (int a = 0; a < 3; a++) rep.check(((R[3] >> (8 * a)) & 0xffu) <= 126u + 127u, "exponent byte in range", s, a);
        rep.check((R[3] >> 24) == 0u, "exponent word's top byte is zero", s);
        bool anyInternal = false;
        for (int j = 0; j < 8; j++) {
            const uint32_t meta = metaOf(R, j);
            if (!meta) continue;
            double lo[3], hi[3];   // exact child planes
            for (int a = 0; a < 3; a++) {
                const double sc = std::ldexp(1.0, (int)((R[3] >> (8 * a)) & 0xffu) - 127);
                const uint32_t ql = (R[8 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                const uint32_t qh = (R[10 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                float p;
                std::memcpy(&p, &R[a], 4);
                lo[a] = (double)p + ql * sc;
                hi[a] = (double)p + qh * sc;
            }
            auto contains = [&](int64_t i) {
                const int64_t k = prim(i);
                if (k < 0) return false;
                for (int a = 0; a < 3; a++)
                    if (!(lo[a] <= (double)A.leafBoxes[(size_t)k * 6 + a] - minQuantum &&
                          hi[a] >= (double)A.leafBoxes[(size_t)k * 6 + 3 + a] + minQuantum))
                        return false;
                return true;
            };
            if (isInternal(meta)) {
                anyInternal = true;
                const int64_t c = (int64_t)R[4] + (meta & 7u);
                rep.check((meta & 7u) == (uint32_t)j, "internal child's slot bits equal its slot", s, j);
                rep.check((meta >> 5) == 1u, "internal child's hit bit", s, j);
                rep.check(c < bound, "child slot in range", s, c);
                if (!(c < bound)) continue;
                if (visits[(size_t)c]++) {
                    rep.check(false, "node reached once", c, s);
                    continue;
                }
                todo.push_back({c, it.level + 1});
                // every primitive below the child lies inside its planes, the margin to spare
                std::vector<int64_t> sub{c};
                stamp[(size_t)c] = ++walkId;
                while (!sub.empty()) {
                    const int64_t x = sub.back();
                    sub.pop_back();
                    const uint32_t* X = A.nodes + (size_t)x * D;
                    for (int jj = 0; jj < 8; jj++) {
                        const uint32_t m = metaOf(X, jj);
                        if (!m) continue;
                        if (isInternal(m)) {
                            const int64_t y = (int64_t)X[4] + (m & 7u);
                            if (y < bound && stamp[(size_t)y] != walkId) {   // (out of range, cycles: reported by the main walk)
                                stamp[(size_t)y] = walkId;
                                sub.push_back(y);
                            }
                        } else {
                            for (uint32_t q = 0; q < 3 && ((m >> 5) >> q & 1u); q++)
                                rep.check(contains((int64_t)X[5] + (m & 31u) + q), "subtree primitive inside child box", s, j);
                        }
                    }
                }
            } else {
                const uint32_t bits = meta >> 5;
                const uint32_t cnt = bits == 1u ? 1u : (bits == 3u ? 2u : 3u);
                const int64_t first = (int64_t)R[5] + (meta & 31u);
                rep.check(bits == 1u || bits == 3u || bits == 7u, "unary leaf count", s, j);
                rep.check((meta & 31u) + cnt <= 24u, "leaf offset < 24", s, j);
                rep.check(first + cnt <= n, "primitive index in range", s, first);
                res.leaves++;
                if (bits == 1u || bits == 3u || bits == 7u) ranges.push_back({first, (int64_t)cnt});
                for (uint32_t q = 0; q < cnt; q++) rep.check(contains(first + q), "leaf inside box", s, j);
            }
        }
        if (anyInternal) {
            rep.check(R[4] < (1u << 24), "child base fits 24 bits", s, R[4]);
            rep.check((int64_t)R[4] + 8 <= A.slots, "child block ends within the reported slots", s, R[4]);
        }
    }
    // the leaf children's ranges tile [0, n)
    std::sort(ranges.begin(), ranges.end());
    int64_t next = 0;
    for (const auto& r : ranges) {
        rep.check(r.first >= next, "leaf ranges overlap", r.first, next);
        rep.check(r.first <= next, "leaf ranges leave a hole", next, r.first);
        next = std::max(next, r.first + r.second);
    }
    rep.check(next >= n, "leaf ranges leave a hole", next, n);
    rep.check(res.depth == A.depth, "reported depth equals the walk's", A.depth, res.depth);
    return res;
}

}  // namespace widecheck
