// pt_instancing.hpp — host build of an instanced scene's two-level tree (host/pt_instancing.cpp).
//
// One 8-wide tree per mesh (binned SAH over the mesh's objects in object space), a top-level 8-wide
// tree over the instances' world boxes with one entry per leaf, whose leaves become instance records
// (pt_wide8.hpp), all in one node array: the top level from slot 0, then the meshes' trees.  Shading
// records in object space, one per mesh primitive (its shading index g); the hit key is
// instance << gBits | g.  Plain C++ on std::vector: no HIP here; csrc/pt_device.hip uploads the
// result (buildInstanced) and csrc/pt_inst_build.hip reproduces the matrix-dependent boxes on the
// device bit for bit, so the expressions below keep their written order.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "pt.h"
#include "pt_wide8.hpp"

namespace pt {

// One instance, for the device's box kernels (pt_inst_dev.hpp): its mesh's objects, and its
// top-level entries.  An entry is the instance entering its mesh tree at a re-braided sub-root;
// subFirst < 0: a single entry at the mesh root, whose box is the instance's exact box.
// entryCount == 0: an instance of an empty mesh (no box, no entry).
struct InstBoxDesc {
    int32_t objFirst, objCount;
    int32_t entryFirst, entryCount;
    int32_t subFirst;
    int32_t pad[3];
};

// A top-level leaf of an instanced scene: an instance entering its mesh's tree at `slot` (the mesh
// tree's own slot numbering: 0 = its root; relocated with the tree).
struct InstEntry {
    uint32_t inst, mesh, slot;
};
static_assert(sizeof(InstEntry) == 12, "uploaded as 3 dwords per entry (pt::instanceRecords, pt_inst_dev.hpp)");

// Traversal stack entries of the wide kernels (one dword per entry): >= the tree depth; -1: too deep.
int wideStackFor(int depth);

// DevScene::mixLim for a scene whose coordinates and extent are at most m.  Both wide builders
// (host/pt_wide8.cpp, csrc/pt_wide_build.hip) give a node the plane quantum s = 2^e with e the
// larger of ceil(log2(m)) - 18 and ceil(log2(node extent / 251)), so s <= 2^eS with
// eS = ceil(log2(m)) + 1; then |s * 2^24 * inv| < 2^128 (finite) for |inv| <= 2^(103 - eS), and the
// exponent byte + 24 stays below 255 for eS <= 100.  Beyond that, every ray takes the reference order.
float mixLimit(double m);

// Partial re-braiding (Benthin et al. 2017): an instance enters its mesh tree below the root, one
// top-level leaf per internal child of the mesh root, each with its own world box, so the top
// level separates overlapping instances at the mesh's second level.  The child boxes come from the
// root's quantised planes (outward-rounded: they contain the subtrees).  Returns the node's
// internal children {slot, object-space box}; empty when the node has leaf children (then the
// instance enters at the node).
struct SubRoot {
    uint32_t slot;
    double box[6];
};
std::vector<SubRoot> nodeChildren(const Wide8& w, uint32_t slot);
// The entries `levels` wide levels below the root (a node with leaf children stays an entry).
void meshSubRoots(const Wide8& w, uint32_t slot, const double* box, int levels, std::vector<SubRoot>& out);
// Partial re-braiding chosen by surface area (PT_INST_ENTRIES = k > 0): start from the root's
// internal children and repeatedly open the entry of the largest surface area (a node whose children
// are all internal) while the entries stay within k per instance -- the large, overlapping boxes are
// opened, the small ones stay closed (in the spirit of Benthin et al. 2017's SAH-driven re-braiding).
void meshSubRootsBudget(const Wide8& w, size_t budget, std::vector<SubRoot>& out);

// What a build reads.  The full build (buildInstancedTree) reads all of it; instanceRecords and
// instanceScalars only the meshes' counts and the instances.
struct InstancedIn {
    const pt_object* objs;       // every mesh's objects, object space
    const int64_t* meshFirst;    // per mesh: its range of `objs`
    const int64_t* meshCount;
    int nMeshes;
    const pt_instance* inst;
    int64_t nInst;
    const float* mats;           // 8 floats per material, the device layout pt_scene_create writes
    int64_t nmat;
    bool dynamic;                // lay out for pt_scene_update_instances (reach x 2, top region at its cap)
    int rebraid;                 // PT_INST_REBRAID (0..3 levels) and PT_INST_ENTRIES (> 0: the entry
    int entryBudget;             // budget instead), read by the caller
    float farExt;                // the kernels' instFar line in world extents (kInstFarExt, pt_render_plan.hpp)
};

// The world-to-object transform of one instance, in double and rounded to the fp32 rows the
// kernels read, and its class (1: identity, 2: translation only, 0: general).  False for a singular
// matrix (|det| <= 1e-30 or not finite).  The one place these are computed: a scene rebuilt after
// pt_scene_update_instances and a fresh scene of the same matrices carry the same rows bit for bit.
bool instanceInverse(const pt_instance& I, std::array<float, 12>& minv, std::array<double, 12>& w2o, uint8_t& cls);

// Every instance's transform records: instanceInverse's, and the `winst` entry the kernels read
// ({world-to-object rows, objBase, class}).
struct InstRecords {
    std::vector<std::array<float, 12>> minv;
    std::vector<uint8_t> ident;   // 1: identity, 2: translation only, 0: general
    std::vector<float> winst;
    std::vector<std::array<double, 12>> w2o;   // world-to-object, double
};
int instanceRecords(const InstancedIn& in, InstRecords& R);   // PT_OK, or fail(PT_ERR_INVALID, ..) on a singular matrix

// The scene scalars that follow from the world box (its centre and largest extent: instFar's
// region, camFar; mixLim), and the reach of world ray origins into each mesh's object space.
// Origins within farExt world extents of the centre (farther camera rays are moved up to the
// world box first, renderKernelWF<.., INST>) map into object space within `reach` of the origin; a
// mesh tree's plane quantum is taken against that reach, not the mesh's own size, so its outward
// margin (wideHits) holds for every ray that enters it.
struct InstScalars {
    float ce[4];   // pt_scene::sceneCE
    float mixLim;
};
void instanceScalars(const InstancedIn& in, const double* wmn, const double* wmx, const std::vector<std::array<double, 12>>& w2o,
                     InstScalars& out, std::vector<double>& reach);

// An instance record (pt_wide8.hpp) for entry e of ctx->entries; dword 4 is the slot in the mesh
// tree's own numbering and dword 6 the mesh, until the layout is known (buildInstancedTree).
struct InstRecCtx {
    const std::vector<std::array<float, 12>>* minv;
    const std::vector<uint8_t>* ident;   // 1: identity, 2: translation only, 0: general
    const std::vector<InstEntry>* entries;
};
void writeInstanceRecord(uint32_t e, uint32_t* dst, void* ctx);

// The top level: an 8-wide tree over the entries' world boxes, one entry per leaf, its leaves
// turned into instance records (the mesh tree's base slot is added by the caller).
bool instanceTop(const InstRecords& rec, const std::vector<InstEntry>& entries, const float* eboxes, Wide8& top, std::string& err);
// Node slots of a top level over n entries, at most: every node has one block of 8 child slots
// (internal children and instance records share it) and stands for at least one internal node of
// the binary tree, of which there are n - 1.
int64_t instanceTopSlots(int64_t n);

// The full build's result: the arrays the kernels read, and the scene scalars.
struct InstancedTree {
    std::vector<uint32_t> nodes, prims, shade;   // kW8NodeDwords per slot; 12 dwords per primitive (never empty)
    std::vector<float> winst;                    // 16 floats per instance (InstRecords::winst)
    int gBits = 0;                               // hit key = instance << gBits | shading index
    int depth = 0;                               // stack entries: top levels, the marker, the mesh's levels
    int maxDepthB = 0;                           // deepest mesh tree
    float sceneCE[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mixLim = -1.0f;
    std::vector<double> reach;                   // per mesh: the reach its tree's planes were quantised for
    std::vector<InstEntry> entries;              // the top level's entries, instances in order
    std::vector<uint32_t> meshRoot;              // per mesh: its root's slot in `nodes`
    uint32_t topCap = 0;                         // node slots of the top level's region (dynamic: its upper bound)
    // dynamic only: the inputs of the later, matrix-only builds (rebuildInstancedTop, pt_device.hip)
    std::vector<InstBoxDesc> desc;               // per instance
    std::vector<double> subBoxes;                // the re-braided sub-roots' object-space boxes (never empty)
    std::vector<uint32_t> entryPrims, entryRank; // the device top-level build's records {.., entry} and identity ranks
};
int buildInstancedTree(const InstancedIn& in, InstancedTree& out);   // PT_OK, or fail(code, message)

}  // namespace pt
