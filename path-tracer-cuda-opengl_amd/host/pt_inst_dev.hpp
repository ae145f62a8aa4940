// pt_inst_dev.hpp — the matrix-dependent boxes of an instanced scene, on the device
// (csrc/pt_inst_build.hip).
//
// After pt_scene_update_instances the mesh trees, primitive records and shading records of the
// two-level tree stay as they are; what changes with the matrices is small except for one part: the
// exact world box of every instance, which takes every vertex of its mesh through the matrix in
// fp64 (C5-instanced: 3.1 M vertex transforms).  That part, and the world boxes of the top-level
// entries derived from it, are computed here, in the host's operation order (buildInstancedTree,
// host/pt_instancing.cpp; -ffp-contract=off on both sides), so the boxes equal the host's bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt.h"
#include "pt_instancing.hpp"   // InstBoxDesc: one instance's objects and top-level entries

namespace pt {

struct InstBoxIn {
    const pt_object* objs;     // the scene's objects (object space)
    const float* m;            // n x 12: the instances' matrices (pt_instance::m)
    const InstBoxDesc* desc;   // n
    const double* sub;         // sub-root boxes in object space, 6 doubles each {min xyz, max xyz}
    int64_t n;
};

// ibox: n x 6 doubles, the exact world box of each instance {min xyz, max xyz};
// ebox: per entry 6 floats, its world box clipped to the instance's and rounded outward.
hipError_t instanceBoxes(const InstBoxIn& in, double* ibox, float* ebox, hipStream_t stream);

// The leaf children of a top level built by WideDevBuilder::buildTop (node slots [0, slots), zeroed
// before the build) -> instance records in their nodes' child blocks.  wprims: the builder's
// leaf-order entry records (dword 7 = the entry); entries: nEntries x {instance, mesh, sub-root slot
// in the mesh tree's own numbering}; winst: 16 floats per instance {world-to-object rows, objBase,
// class}; meshRoot: per mesh, its root's slot in the node array; *err |= bits on a malformed node.
hipError_t instanceRecords(uint32_t* nodes, uint32_t slots, const uint32_t* wprims, const uint32_t* entries, uint32_t nEntries,
                           const float* winst, const uint32_t* meshRoot, uint32_t* err, hipStream_t stream);

// The sampled lights of an instanced scene built with PT_BVH_LIGHTS (pt.h: the rule): nLights records
// {v0}{e1}{e2}{E} of 4 float4, one per (instance, emissive triangle of its mesh), in world space.
struct InstLightIn {
    const pt_object* objs;    // the scene's objects (object space)
    const float* mats;        // the device's material records, 8 floats each (the albedo slot first: E)
    const float* m;           // nInst x 12: the instances' matrices
    const uint32_t* first;    // nInst + 1: each instance's first record; first[nInst] = nLights
    const uint32_t* src;      // nInst: where the instance's mesh's run starts in `obj`
    const uint32_t* obj;      // the emissive triangles' object indices, mesh by mesh, in object order
    uint32_t nInst, nLights;
};
hipError_t instanceLights(const InstLightIn& in, float4* lights, hipStream_t stream);

}  // namespace pt
