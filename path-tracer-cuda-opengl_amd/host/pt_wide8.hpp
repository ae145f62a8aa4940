// pt_wide8.hpp — host build of the compressed 8-wide BVH traversed by the wide render kernel.
//
// The reference traverses its binary LBVH depth first (RenderManager::hitBvh,
// utils/render_manager.h:86-135).  The wide tree is an acceleration structure of this build
// only: a binned-SAH binary tree over the same primitive records, collapsed to 8 children per
// node, child boxes quantised outward to 8 bits per plane.  It changes which nodes are visited
// and in which order, never which primitive is the closest hit ("Wide tree").
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt.h"

namespace pt {

#ifndef PT_NODE_DWORDS
#define PT_NODE_DWORDS 20   // a node slot: the 80-B record; 32 pads each slot to one 128-B cache line (A/B builds)
#endif
constexpr int kW8NodeDwords = PT_NODE_DWORDS;   // node slot in dwords: 80-B record (layout in pt_wide8.cpp) + padding
static_assert(kW8NodeDwords == 20 || kW8NodeDwords == 32, "node slots of 80 or 128 B");
constexpr int kW8PrimDwords = 12;   // 48-B primitive record
constexpr int kW8BoxFloats = 8;     // exact-box record per rank: {mn.x, mx.x, mn.y, mx.y} {mn.z, mx.z, 0, 0}

// The exact box of a triangle record {v0, .}{v1, .}{v2, .} as the reference's leaf test sees it
// (min / max of the vertices in their order, utils::unionPoints), in the render kernels' slab
// layout.  Only triangle-only scenes read it (a sphere record gives a box nobody uses).
inline void exactTriBox(const float* rec, float* out) {
    for (int a = 0; a < 3; a++) {
        out[2 * a] = std::fmin(std::fmin(rec[a], rec[4 + a]), rec[8 + a]);
        out[2 * a + 1] = std::fmax(std::fmax(rec[a], rec[4 + a]), rec[8 + a]);
    }
    out[6] = out[7] = 0.0f;
}

// The 48-byte primitive record of an object, {v0, mat}{v1, id}{v2, 0} or {c, mat}{r, 0, 0, id}{0, 0, 0, 1},
// and its box {min xyz, max xyz}, as the LBVH's leafGatherKernel writes them (pt_device.hip): the
// input of buildWide8.  id: what the caller numbers the object by (the scene's object id, or the
// object within its mesh).
inline void primRecord(const pt_object& o, uint32_t id, uint32_t* rec, float* box) {
    float f[kW8PrimDwords] = {};
    if (o.type == PT_SPHERE) {
        f[0] = o.v[0]; f[1] = o.v[1]; f[2] = o.v[2]; f[4] = o.v[3];
        const float rr = std::fabs(o.v[3]);
        for (int a = 0; a < 3; a++) { box[a] = o.v[a] - rr; box[3 + a] = o.v[a] + rr; }
    } else {
        for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) f[4 * v + a] = o.v[3 * v + a];
        for (int a = 0; a < 3; a++) {
            box[a] = std::fmin(std::fmin(o.v[a], o.v[3 + a]), o.v[6 + a]);
            box[3 + a] = std::fmax(std::fmax(o.v[a], o.v[3 + a]), o.v[6 + a]);
        }
    }
    std::memcpy(rec, f, sizeof(f));
    rec[3] = (uint32_t)o.mat;
    rec[7] = id;
    rec[11] = o.type == PT_SPHERE ? 1u : 0u;
}

// Edge form of n wide-order triangle records {v0, rank}{v1, .}{v2, .} -> {v0, rank}{e1, .}{e2, .}
// with e1 = v1 - v0, e2 = v2 - v0: the two subtractions every triangle test starts with
// (cuda_object.h:66-67), done once per triangle instead of once per test.  Each component is one
// IEEE fp32 subtraction (denormals kept), so a test that starts from the edges computes the same
// bits.  Word 3 of each 16-B word is copied.  Only triangle-only, non-instanced scenes have the
// array (DevScene::wprims of their render launches); `out` may not alias `prims`.
inline void edgeTriRecords(const uint32_t* prims, int64_t n, uint32_t* out) {
    for (int64_t k = 0; k < n; k++) {
        const uint32_t* src = prims + (size_t)k * kW8PrimDwords;
        uint32_t* dst = out + (size_t)k * kW8PrimDwords;
        float v[kW8PrimDwords];
        std::memcpy(v, src, sizeof(v));
        std::memcpy(dst, src, sizeof(v));
        for (int a = 0; a < 3; a++) {
            const float e1 = v[4 + a] - v[a], e2 = v[8 + a] - v[a];
            std::memcpy(dst + 4 + a, &e1, 4);
            std::memcpy(dst + 8 + a, &e2, 4);
        }
    }
}

// The builders' smallest plane quantum is 2^-kW8EminShift of the larger of the scene's extent and
// its coordinates; the traversal sends a ray whose origin lies farther than kW8FarExt scene extents
// from the scene's centre to the reference-order query instead of the quantised test (wideFar,
// pt_device.hip).  The two move together: the planes' outward margin (>= 2^-shift of the scale)
// must stay beyond the rounding of the ray's plane distances (about 2^-21.6 of |p - o|), which
// grows with the far line.  The bound below restates that argument (the wideHits comment) at the
// shipped pair, shift 18 with 8 extents -- it is no new measurement: a finer quantum needs a
// nearer far line by the same factor.
#ifndef PT_WIDE_EMIN_SHIFT
#define PT_WIDE_EMIN_SHIFT 18
#endif
#ifndef PT_WIDE_FAR_EXT
#define PT_WIDE_FAR_EXT 8.0f
#endif
constexpr int kW8EminShift = PT_WIDE_EMIN_SHIFT;
constexpr float kW8FarExt = PT_WIDE_FAR_EXT;
static_assert(kW8EminShift >= 0 && kW8EminShift < 31 &&
                  (double)kW8FarExt * (double)(1u << kW8EminShift) <= 8.0 * (double)(1u << 18),
              "PT_WIDE_EMIN_SHIFT and PT_WIDE_FAR_EXT move together: far line * 2^shift <= 8 * 2^18");

struct Wide8 {
    std::vector<uint32_t> nodes;   // kW8NodeDwords per node slot; slot 0 = root
    std::vector<uint32_t> prims;   // kW8PrimDwords per primitive, in traversal (leaf) order
    int depth = 0;                 // wide levels, root = 1 (= traversal stack entries needed)
    int64_t usedNodes = 0;         // slots holding a node (children blocks are 8 slots, sparse)
    int64_t leaves = 0;
};

// prims: n leaf-order (Morton) primitive records of kW8PrimDwords dwords (the device `prims`
// array: {v0, mat}{v1, objID}{v2, sphere flag} or {c, mat}{r, 0, 0, objID}{0, 0, 0, 1});
// boxes: n x {min xyz, max xyz}; rank: per leaf k its position in the reference's traversal
// order (referenceRanks).  The output records carry the rank in place of the material id
// ({v0, rank}...): ties between equal hit distances are decided by it, and it indexes the wide
// kernels' shading records.  Returns false with `err` set when the tree exceeds the encoding
// limits.
// scaleFloor: the plane quantum is at least 2^-18 of max(scaleFloor, the tree's extent and
// coordinates) -- the distance up to which ray origins keep the boxes' outward margin (instanced
// meshes: the world's reach in object space).
bool buildWide8(const uint32_t* prims, const float* boxes, const uint32_t* rank, int64_t n, Wide8& out,
                std::string& err, double scaleFloor = 0.0);
// buildWide8 with at most maxLeaf (1..3) primitives per leaf child (instancing's top level: one
// instance per leaf).
bool buildWide8Leaf(const uint32_t* prims, const float* boxes, const uint32_t* rank, int64_t n, int maxLeaf,
                    Wide8& out, std::string& err, double scaleFloor = 0.0);

// Instancing (two-level tree in one node array).  Record of an instance node, kW8NodeDwords:
//   [0] 1 if the transform is the identity (the ray is not transformed), [1] 1 if it only
//   translates (the origin moves, the direction stays), [2] 0,
//   [3] kW8InstanceFlag (never a valid exponent word: byte 3 of a node's exponents is 0),
//   [4] the instance's bottom-level root slot, [5] the instance id, [6..7] 0,
//   [8..19] the world-to-object transform, 3 rows of {m0, m1, m2, t} (fp32).
constexpr uint32_t kW8InstanceFlag = 0xff000000u;
// Relocate a tree built on its own into a shared node / primitive array: child bases += nodeBase,
// primitive bases += primBase.
void relocateWide8(Wide8& w, uint32_t nodeBase, uint32_t primBase);
// Turn the leaf children of a top-level tree built with buildWide8Leaf(.., 1, ..) over instance
// boxes into internal children whose slots hold instance records: instanceOf(prim record) gives
// the instance id of a leaf's primitive record, record(id, dst) writes its 20-dword record.
// Nodes without a child block get one.  Returns false with err set past the encoding limits.
bool instanceLeaves(Wide8& top, uint32_t (*instanceOf)(const uint32_t* primRecord),
                    void (*record)(uint32_t id, uint32_t* dst, void* ctx), void* ctx, std::string& err);

// The order in which RenderManager::hitBvh (render_manager.h:105-133) would test the leaves of
// the binary LBVH if every box passed: at a node, its leaf children (left, then right), then the
// right subtree, then the left one (the left child is pushed first, so the right one is popped
// first).  refs: per internal node its two child refs (bit 31 = leaf, low 30 bits = leaf k).
// Returns rank[k].
std::vector<uint32_t> referenceRanks(const uint32_t* leftRef, const uint32_t* rightRef, size_t stride, int64_t n);

}  // namespace pt
