// pt_device.hip — MI355X (gfx950) device path: LBVH build, closest-hit traversal, render.
//
// Hot path re-designed for CDNA4:
//  * render: one lane per pixel of an 8x8 tile (one wave per workgroup), path regeneration
//    (a lane whose path ends starts its next sample in the same loop iteration, so no lane
//    idles between samples), per-lane XORWOW state in registers, coalesced SoA state I/O.
//  * traversal: BVH2 whose internal-node record holds BOTH child boxes + child refs (64 B,
//    four dwordx4 loads per visit, one 64-B segment); leaves are folded into the parent's
//    child refs; the traversal stack lives in LDS, lane-interleaved (conflict-free).
//  * primitives are stored in Morton (leaf) order, 48 B each ({v0,v1,v2} / {c,r}: the exact
//    object box is recomputed from them); a 48-B shading record per primitive (normal or
//    sphere centre/radius + the material inline) is read once per closest hit, in one round trip.
//  * LBVH: Karras hierarchy kernel + atomic-counter bottom-up refit with tight boxes.
// All arithmetic follows the reference's operation order and is compiled with
// -ffp-contract=off, so results are bit-identical to oracle/ (the CPU restatement).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <memory>
#include <string>
#include <vector>

#include "../host/pt_denoise_dev.hpp"
#include "../host/pt_temporal_dev.hpp"
#include "../host/pt_error.hpp"
#include "../host/pt_host.hpp"
#include "../host/pt_inst_dev.hpp"
#include "../host/pt_instancing.hpp"
#include "../host/pt_render_plan.hpp"
#include "../host/pt_wide8.hpp"
#include "../host/pt_wide_dev.hpp"
#include "pt.h"
#include "pt_math.hpp"

using pt::fail;
// The launch plan's knobs and helpers that this file reads as well (host/pt_render_plan.hpp)
using pt::critFor;
using pt::envCount;
using pt::envInt;
using pt::kInstFarExt;
using pt::kTaskPool;
using pt::stackFor;

#include "pt_prims.hpp"   // radixSortPairs (pt_sort.hip)

namespace pt {
int launchCompatWide(int stack, const void* params, hipStream_t st);   // pt_compat.hip
int compatWideWavesPerCU(int stack, bool tri, int& n);                  // pt_compat.hip
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

namespace {

constexpr int kWave = 64;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kSphereBit = 0x40000000u;
constexpr uint32_t kPrimMask = 0x3fffffffu;
constexpr int kJumpMats = 32;                    // XORWOW 2^(67+k) jump matrices, k < 32
constexpr int kNumCounters = 32;                 // per-scene u64 counters: work counts, error word, diagnostics

// ------------------------------------------------------------------------ device structs
struct DevScene {
    const float4* nodes;     // 4 x float4 per internal node: child boxes as (min, max) pairs per axis, refs (nodeBoxIdx)
    const float4* prims;     // 3 x float4 per primitive (leaf order)
    const float4* shade;     // 3 x float4 per primitive: {n | c, r} {albedo, fuzz} {ir, type | sphere << 16, mat, obj}
    const float4* mats;      // 2 x float4 per material
    const float4* wnodes;    // compressed 8-wide nodes, 5 x float4 each (renderKernelWF<.., WIDE>; host/pt_wide8.cpp)
    const float4* wprims;    // primitive records in wide-tree leaf order, {v0, rank} {v1, objID} {v2, sphere}; the render
                             // launches of a triangle-only, non-instanced scene get its edge-form records here
                             // instead, {v0, rank} {v1 - v0, objID} {v2 - v0, 0} (pt_scene::wtris, wideTestTri)
    const float4* wshade;    // shading records in reference rank order (wide kernels)
    const float4* wbox;      // exact triangle boxes in rank order, {mn.x, mx.x, mn.y, mx.y} {mn.z, mx.z, 0, 0} (deferredRedo)
    const uint32_t* rankOf;  // leaf k -> its rank in the reference's traversal order
    const int* iparent;      // parent of each internal LBVH node (-1 for the root)
    unsigned int* err;       // set (never cleared in-kernel) when a traversal guard trips
    int nprims;
    int hasSpheres;          // 0: triangles only (the wide kernels' LEAF tests drop the sphere tie rules)
    float cx, cy, cz, ext;   // tight scene box: centre and largest extent (the wide kernels' far-origin test)
    float mixLim;            // largest finite |1 / d| component the MIX plane arithmetic takes (wideHits, mixUnsafe)
    // instanced scenes (renderKernelWF<.., INST>): per instance {world-to-object rows r0, r1, r2}
    // {objBase, identity, 0, 0}; a hit's key is instance << gBits | its primitive's shading index
    const float4* winst;
    int gBits;
};
// Instancing: the stack entry that returns a lane from an instance's bottom-level tree to the world
// (a child base of 2^24 - 1 never exists); the exponent word of an instance record (pt_wide8.hpp).
constexpr uint32_t kInstMarker = 0xffffffffu;
constexpr uint32_t kInstFlag = 0xff000000u;

struct DevCamera {
    float3 pos, ll, hor, ver;
    float3 right, up;
    float lens;   // lens radius (aperture / 2); 0: a pinhole, no lens draws
};


struct Counters {
    uint32_t rays, visits, tris, spheres;
};

// ------------------------------------------------------------------------ math helpers
// Exact restatements of utils/vec3.h operators (no contraction: -ffp-contract=off).
__device__ __forceinline__ float3 f3(float a, float b, float c) { return make_float3(a, b, c); }
__device__ __forceinline__ float3 add(float3 a, float3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float3 sub(float3 a, float3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 mul(float3 a, float3 b) { return f3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ float3 scale(float t, float3 v) { return f3(t * v.x, t * v.y, t * v.z); }
__device__ __forceinline__ float3 neg(float3 v) { return f3(-v.x, -v.y, -v.z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 cross3(float3 u, float3 v) {
    return f3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
__device__ __forceinline__ float len2(float3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
__device__ __forceinline__ float3 divs(float3 v, float t) { return scale(rcpRN(t), v); }
__device__ __forceinline__ float3 normalize3(float3 v) {
    float l = sqrtf(len2(v));
    if (l == 0.0f) return f3(0.0f, 0.0f, 0.0f);
    return divs(v, l);
}
__device__ __forceinline__ float3 xyz(float4 v) { return f3(v.x, v.y, v.z); }

// ------------------------------------------------------------------------ XORWOW
struct Xorwow {
    uint32_t d, v0, v1, v2, v3, v4;
    __device__ __forceinline__ uint32_t next() {   // curand(curandStateXORWOW*)
        uint32_t t = v0 ^ (v0 >> 2);
        v0 = v1; v1 = v2; v2 = v3; v3 = v4;
        // the three-way XOR in one v_bitop3_b32 (gfx950): six VALU per draw instead of seven
        v4 = __builtin_amdgcn_bitop3_b32(v4, v4 << 4, t ^ (t << 1), 0x96);
        d += 362437u;
        return v4 + d;
    }
    // curand_uniform: x * 2^-32 + 2^-33 in (0, 1] (one exact FMA, pt_math.hpp)
    __device__ __forceinline__ float uniform() { return uniformOf(next()); }
    // 2 * (uniform() - 0.5f): the unit-sphere coordinates (one exact FMA, pt_math.hpp)
    __device__ __forceinline__ float centered2() { return centered2Of(uniform()); }
    // centered2() three times (x, y, z in order): the same draws with the state's rotation by three
    // words written out, so a rejection-loop trial moves two state words (v3, v4), not five
    __device__ __forceinline__ float3 centered2x3() {
        uint32_t t0 = v0 ^ (v0 >> 2), t1 = v1 ^ (v1 >> 2), t2 = v2 ^ (v2 >> 2);
        // (empty asm: an order for the scheduler -- the old v0, v1, v2 are dead before the new words
        // are written, and d steps after its uses -- so the new words take the old ones' registers)
        asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2));
        // (the two moves written out where the old v0 and v1 are free: copies left to the register
        // allocator land at the loop's ends and take a third and a fourth to get there)
        uint32_t r0, r1;
        asm volatile("v_mov_b32 %0, %1" : "=v"(r0) : "v"(v3));
        asm volatile("v_mov_b32 %0, %1" : "=v"(r1) : "v"(v4));
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32(v4, v4 << 4, t0 ^ (t0 << 1), 0x96);
        const uint32_t n1 = __builtin_amdgcn_bitop3_b32(n0, n0 << 4, t1 ^ (t1 << 1), 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32(n1, n1 << 4, t2 ^ (t2 << 1), 0x96);
        uint32_t x0 = n0 + (d + 362437u), x1 = n1 + (d + 2u * 362437u);
        asm volatile("" : "+v"(x0), "+v"(x1));
        d += 3u * 362437u;
        v0 = r0; v1 = r1; v2 = n0; v3 = n1; v4 = n2;
        return f3(centered2Of(uniformOf(x0)), centered2Of(uniformOf(x1)), centered2Of(uniformOf(n2 + d)));
    }
};

// Sample mode stream of (pixel p, sample s): one Philox4x32-10 block (Salmon et al. 2011)
// with key = seed and counter = {s, p_lo, p_hi, "SAMP"} seeds a XORWOW state, whose draws
// then cost a few shifts each (the reference's generator family, curand_uniform mapping).
// Any sample of any pixel starts anywhere, in one block of work.
// PEEL (the step kernels' camera-ray site): rounds 1 and 2 written out with the counter's zero word
// folded (the loop's trip count hides it from the compiler).  Round 1: c2 = 0, so its product is 0
// -- no second multiply, n0 = c1 ^ k0, and the next c1 = 0.  Round 2: that zero c1 drops out of n0.
// The same words as ten loop rounds; the simple kernel keeps the loop alone (the written-out rounds
// cost it two VGPRs).
template <bool PEEL = false>
__device__ __forceinline__ Xorwow sampleStream(uint32_t k0, uint32_t k1, uint32_t sample, uint32_t pixel) {
    uint32_t c0 = sample, c1 = pixel, c2 = 0u, c3 = 0x53414D50u;
    if constexpr (PEEL) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * sample;
        const uint32_t a0 = pixel ^ k0, a2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), 0x53414D50u, k1, 0x96);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
        const uint64_t q0 = (uint64_t)0xD2511F53u * a0, q1 = (uint64_t)0xCD9E8D57u * a2;
        c0 = (uint32_t)(q1 >> 32) ^ k0;
        c1 = (uint32_t)q1;
        c2 = __builtin_amdgcn_bitop3_b32((uint32_t)(q0 >> 32), (uint32_t)p0, k1, 0x96);
        c3 = (uint32_t)q0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    // (the loop alone: pairs of rounds -- no register moves, and a full unroll raised the camera-ray
    // site's pressure; after the written-out rounds the remaining eight unroll at no register's cost
    // and drop the loop's counter, compare and four branches per stream)
#pragma unroll(PEEL ? 8 : 2)
    for (int r = PEEL ? 2 : 0; r < 10; r++) {
        // one 32 x 32 -> 64 multiply per word (v_mad_u64_u32) instead of mul_hi + mul_lo
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        // (three-way XORs as one v_bitop3_b32 each)
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96), n2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Xorwow{c3, c0, c1, c2, c3 ^ 0x6C078965u, c0 ^ c1 ^ 0x2545F491u};
}

// ------------------------------------------------------------------------ traversal
// aabb::hit (aabb.h:21-34): per axis t0=(min-o)*inv, t1=(max-o)*inv, swap if inv<0,
// tmin=max(tmin,t0), tmax=min(tmax,t1); miss if tmax<tmin.  The ternaries of the reference
// keep the old bound on NaN, which is exactly maxNum/minNum (v_max_f32 / v_min_f32).
// SlabHit also returns the entry distance lo = max(tmin, near planes).  For a box that
// passed with tmax = T, the same test with any tmax' <= T fails iff tmax' < lo: hi(T') =
// fminf(T', far planes) and fminf ignores NaN, so hi(T') < lo <=> T' < lo or far < lo, and
// the latter is false because the box passed.  (lo is never NaN: fmaxf(tmin, NaN) = tmin.)
struct SlabHit { bool hit; float lo; };

// Internal node record, 16 floats (4 x float4).  Each child box is stored as one (min, max)
// pair per axis, so every pair sits in an aligned 64-bit register pair and the six slab
// planes of a child cost three packed subtracts and three packed multiplies
// (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations, two per instruction):
//   [0..5]  left  {mnx, mxx, mny, mxy, mnz, mxz}     [6..11] right {mnx, mxx, mny, mxy, mnz, mxz}
//   [12] left ref  [13] right ref  [14..15] unused
__host__ __device__ constexpr int nodeBoxIdx(int child, int axis, int isMax) { return 6 * child + 2 * axis + isMax; }

typedef float v2f __attribute__((ext_vector_type(2)));

// slabLo on a box given as (min, max) pairs per axis (the node record layout).
__device__ __forceinline__ SlabHit slabPair(v2f X, v2f Y, v2f Z, float3 o, float3 inv, float tmin, float tmax) {
    const v2f tx = (X - o.x) * inv.x, ty = (Y - o.y) * inv.y, tz = (Z - o.z) * inv.z;
    float nx = inv.x < 0.0f ? tx.y : tx.x, fx = inv.x < 0.0f ? tx.x : tx.y;
    float ny = inv.y < 0.0f ? ty.y : ty.x, fy = inv.y < 0.0f ? ty.x : ty.y;
    float nz = inv.z < 0.0f ? tz.y : tz.x, fz = inv.z < 0.0f ? tz.x : tz.y;
    float lo = fmaxf(fmaxf(fmaxf(tmin, nx), ny), nz);
    float hi = fminf(fminf(fminf(tmax, fx), fy), fz);
    return SlabHit{!(hi < lo), lo};
}
// Both child boxes of a node record at once (the 12 plane distances first, then the selects).
struct SlabHit2 { SlabHit l, r; };
__device__ __forceinline__ SlabHit2 slabBoth(float4 a, float4 b, float4 q, float3 o, float3 inv, float tmin,
                                             float tmax) {
    const v2f lx = (v2f{a.x, a.y} - o.x) * inv.x, ly = (v2f{a.z, a.w} - o.y) * inv.y,
              lz = (v2f{b.x, b.y} - o.z) * inv.z;
    const v2f rx = (v2f{b.z, b.w} - o.x) * inv.x, ry = (v2f{q.x, q.y} - o.y) * inv.y,
              rz = (v2f{q.z, q.w} - o.z) * inv.z;
    const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
    SlabHit2 h;
    {
        const float lo = fmaxf(fmaxf(fmaxf(tmin, sx ? lx.y : lx.x), sy ? ly.y : ly.x), sz ? lz.y : lz.x);
        const float hi = fminf(fminf(fminf(tmax, sx ? lx.x : lx.y), sy ? ly.x : ly.y), sz ? lz.x : lz.y);
        h.l = SlabHit{!(hi < lo), lo};
    }
    {
        const float lo = fmaxf(fmaxf(fmaxf(tmin, sx ? rx.y : rx.x), sy ? ry.y : ry.x), sz ? rz.y : rz.x);
        const float hi = fminf(fminf(fminf(tmax, sx ? rx.x : rx.y), sy ? ry.x : ry.y), sz ? rz.x : rz.y);
        h.r = SlabHit{!(hi < lo), lo};
    }
    return h;
}
// Both child boxes of a node record (a, b, q = its first three float4s).
__device__ __forceinline__ SlabHit slabLeft(float4 a, float4 b, float3 o, float3 inv, float tmin, float tmax) {
    return slabPair(v2f{a.x, a.y}, v2f{a.z, a.w}, v2f{b.x, b.y}, o, inv, tmin, tmax);
}
__device__ __forceinline__ SlabHit slabRight(float4 b, float4 q, float3 o, float3 inv, float tmin, float tmax) {
    return slabPair(v2f{b.z, b.w}, v2f{q.x, q.y}, v2f{q.z, q.w}, o, inv, tmin, tmax);
}

// Primitive record (leaf order), 3 x float4:
//   triangle {v0, mat} {v1, objID} {v2, 0}        sphere {c, mat} {r, 0, 0, objID} {0, 0, 0, 1}
struct Prim { float4 p0, p1, p2; };
// Raw gfx9 buffer resource over a device array (stride 0, DATA_FORMAT_32): per-lane loads then
// take a 32-bit offset instead of 64-bit address arithmetic.  Arrays stay below 4 GB (< 2^26
// primitives / nodes, pt_scene_create).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rawRsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1 /* 4 GB of records */, 0x00020000);
}
// Integer products by small constants as full-rate shifts.  v_mul_lo_u32 (and the 64-bit
// v_mad_u64_u32) issue at a quarter of the VALU rate; LLVM folds `(x << a) + (x << b)` back into
// a multiply and lowers it with v_mul_lo_u32, so one shift is done in an (empty-effect) asm
// statement the folder cannot see through.
template <int S>
__device__ __forceinline__ uint32_t shlOpaque(uint32_t x) {
    uint32_t t;
    asm("v_lshlrev_b32 %0, %1, %2" : "=v"(t) : "i"(S), "v"(x));
    return t;
}
// byte offset of node slot x (80-B slots: x < 2^26; 128-B slots, PT_NODE_DWORDS 32: x < 2^25)
__device__ __forceinline__ uint32_t mul80(uint32_t x) {
    if constexpr (pt::kW8NodeDwords == 32) return x << 7;
    return shlOpaque<6>(x) + (x << 4);
}
__device__ __forceinline__ uint32_t mul48(uint32_t x) { return shlOpaque<5>(x) + (x << 4); }   // x < 2^27
// A wave total (the render kernels' work counters) plus a wave-uniform count, in a scalar register.
// Written as the instruction: a plain `acc += n` of two uniform values is selected as a v_add_u32
// on a VGPR accumulator that then lives for the whole kernel (one VALU per update and one of the 96
// registers per counter), and a readfirstlane around the sum does not change that.
__device__ __forceinline__ void waveCount(uint32_t& acc, uint32_t n) {
    asm("s_add_u32 %0, %0, %1" : "+s"(acc) : "s"(n) : "scc");
}
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

__device__ __forceinline__ Prim loadPrim(const DevScene& S, uint32_t k) {
    const float4* p = S.prims + 3 * (size_t)k;
    return Prim{p[0], p[1], p[2]};
}

// CudaObj::hit (cuda_object.h:44-92): returns the accepted t (> tmin > 0), or -1 on a miss.
// `closest` is the current t_max.  Values are returned, never written through references, so
// the compiler keeps every traversal variable in registers.
__device__ __forceinline__ float primHitT(const Prim& q, bool sphere, float3 o, float3 d, float tmin, float closest) {
    if (sphere) {
        float3 oc = sub(o, xyz(q.p0));
        float r = q.p1.x;
        float a = len2(d);
        float half_b = dot3(oc, d);
        float cc = len2(oc) - r * r;
        float disc = half_b * half_b - a * cc;
        if (disc < 0.0f) return -1.0f;
        float sq = sqrtf(disc);
        float root = (-half_b - sq) / a;
        if (root < tmin || closest < root) {
            root = (-half_b + sq) / a;
            if (root < tmin || closest < root) return -1.0f;
        }
        return root;
    }
    const float3 v0 = xyz(q.p0);
    float3 e1 = sub(xyz(q.p1), v0), e2 = sub(xyz(q.p2), v0);
    float3 s1 = cross3(d, e2);
    float det = dot3(s1, e1);
    if (det == 0.0f) return -1.0f;
    float3 s = sub(o, v0);
    float3 s2 = cross3(s, e1);
    float inv = rcpRN(det);
    float t = dot3(s2, e2) * inv;
    float b1 = dot3(s1, s) * inv;
    float b2 = dot3(s2, d) * inv;
    // The reference's strict tests (cuda_object.h:83) without `b1 + b2 <= 0`, which never decides:
    // a sum that is <= 0 is not NaN, so neither term is, and the rounded sum of two positive terms
    // is positive -- one of b1 <= 0, b2 <= 0 already rejected it.  (b1 >= 1 and b2 >= 1 stay: with
    // the other term NaN, the sum test would not see them.)
    if (b1 >= 1.0f || b1 <= 0.0f || b2 >= 1.0f || b2 <= 0.0f || b1 + b2 >= 1.0f || t <= tmin || t >= closest)
        return -1.0f;
    return t;
}

__device__ __forceinline__ void primTest(const DevScene& S, uint32_t ref, float3 o, float3 d, float tmin,
                                         float& closest, int& best, Counters& c) {
    const uint32_t k = ref & kPrimMask;
    const bool sph = (ref & kSphereBit) != 0;
    if (sph) c.spheres++;
    else c.tris++;
    const float t = primHitT(loadPrim(S, k), sph, o, d, tmin, closest);
    if (t >= 0.0f) {
        closest = t;
        best = (int)k;
    }
}

// ------------------------------------------------------------------------ wide tree
// The reference's closest hit does not depend on its traversal order except through ties:
// a primitive is accepted when t < closest (triangle, cuda_object.h:83) or t <= closest
// (sphere, :57-61), and its left-first DFS visits leaves in key order k.  So the reference's
// result over ANY set of visited primitives that contains every primitive it would accept is
// the minimum of (t, tie rank) with ranks: spheres before triangles, spheres by DESCENDING k
// (a later sphere at the same t replaces the earlier hit), triangles by ASCENDING k (a later
// triangle at the same t is rejected).  The wide tree's boxes are conservative (outward-rounded
// planes, pt_wide8.cpp), so every primitive the reference would accept is visited.

// Candidate distance of a primitive independent of the current closest hit: the sphere's
// first root when >= tmin, else its second (the reference tries them in this order against
// [tmin, closest]; the second is never smaller); triangles as primHitT.  -1 on a miss.
__device__ __forceinline__ float primHitAny(const Prim& q, bool sphere, float3 o, float3 d, float tmin) {
    if (sphere) {
        float3 oc = sub(o, xyz(q.p0));
        float r = q.p1.x;
        float a = len2(d);
        float half_b = dot3(oc, d);
        float cc = len2(oc) - r * r;
        float disc = half_b * half_b - a * cc;
        if (disc < 0.0f) return -1.0f;
        float sq = sqrtf(disc);
        float root = (-half_b - sq) / a;
        if (!(root < tmin)) return root;
        root = (-half_b + sq) / a;
        if (!(root < tmin)) return root;
        return -1.0f;
    }
    const float3 v0 = xyz(q.p0);
    float3 e1 = sub(xyz(q.p1), v0), e2 = sub(xyz(q.p2), v0);
    float3 s1 = cross3(d, e2);
    float det = dot3(s1, e1);
    if (det == 0.0f) return -1.0f;
    float3 s = sub(o, v0);
    float3 s2 = cross3(s, e1);
    float inv = rcpRN(det);
    float t = dot3(s2, e2) * inv;
    float b1 = dot3(s1, s) * inv;
    float b2 = dot3(s2, d) * inv;
    if (b1 >= 1.0f || b1 <= 0.0f || b2 >= 1.0f || b2 <= 0.0f || b1 + b2 >= 1.0f || t <= tmin)   // (as primHitT)
        return -1.0f;
    return t;
}

// aabb::hit (aabb.h:21-34) on the primitive's exact box (cuda_object.h:21-42: sphere c -/+ |r|,
// triangle min / max of its vertices): the test the reference's traversal applies to a leaf
// before its primitive test (render_manager.h:107-123).
__device__ __forceinline__ SlabHit refLeafBox(const Prim& q, bool sphere, float3 o, float3 inv, float tmin, float tmax) {
    float mn[3], mx[3];
    if (sphere) {
        const float r = fabsf(q.p1.x);
        mn[0] = q.p0.x - r; mn[1] = q.p0.y - r; mn[2] = q.p0.z - r;
        mx[0] = q.p0.x + r; mx[1] = q.p0.y + r; mx[2] = q.p0.z + r;
    } else {   // utils::unionPoints (aabb.h:68-79); vertices are never NaN, so v_min3 / v_max3
        // give the same planes (up to the sign of a zero, which no slab comparison sees)
        mn[0] = fminf(fminf(q.p0.x, q.p1.x), q.p2.x);
        mn[1] = fminf(fminf(q.p0.y, q.p1.y), q.p2.y);
        mn[2] = fminf(fminf(q.p0.z, q.p1.z), q.p2.z);
        mx[0] = fmaxf(fmaxf(q.p0.x, q.p1.x), q.p2.x);
        mx[1] = fmaxf(fmaxf(q.p0.y, q.p1.y), q.p2.y);
        mx[2] = fmaxf(fmaxf(q.p0.z, q.p1.z), q.p2.z);
    }
    return slabPair(v2f{mn[0], mx[0]}, v2f{mn[1], mx[1]}, v2f{mn[2], mx[2]}, o, inv, tmin, tmax);
}

// Test wide-order primitive record q ({v0, rank}{v1, obj}{v2, sphere}) and keep the minimum of
// (t, tie rank).  `best` = rank | kSphereBit for a sphere, -1 before the first hit.
// The reference only tests a primitive whose exact box passes with the closest hit of that
// moment (aabb::hit, render_manager.h:107-123; a single primitive is the root and has no box
// test, :92-98).  A hit inside its own box (entry lo <= t, as exact arithmetic guarantees) is
// tested by the reference whenever it could matter, in any order.  A grazing hit whose rounded
// box entry lies beyond it (t < lo) is tested only if the closest hit of that moment is >= lo:
// the outcome depends on the order exactly when another candidate's t lies in [t, lo).  Such a
// lane sets `redo` and its query is repeated in the reference's order (traceRefStackless);
// `bestLo` is the current best's window end (its box entry when t < lo, else -inf).
// SPH = false: the scene has no spheres (DevScene::hasSpheres), so neither q nor the current best
// is one and the tie rule reduces to the triangles' ascending rank -- the same decisions with
// fewer instructions.
// This per-candidate form serves scenes with spheres, the instanced kernels (leafBoxes = false) and
// the ray-query kernels; the non-instanced render kernels on triangle-only scenes decide the same
// rule once per query (wideTestTri / deferredRedo below).
template <bool SPH>
__device__ __forceinline__ void wideTest(const Prim& q, float3 o, float3 d, float3 inv, float tmin, float& closest,
                                         int& best, float& bestLo, bool leafBoxes, bool& redo, uint32_t keyHi = 0u) {
    const bool sph = SPH && __float_as_uint(q.p2.w) != 0u;
    const float t = primHitAny(q, sph, o, d, tmin);
    if (t >= 0.0f) {
        // (instanced scenes: the instance id above the shading index, keyHi = instance << gBits)
        const int k = (int)(keyHi | __float_as_uint(q.p0.w));
        const bool none = best < 0, bSph = SPH && (best & (int)kSphereBit) != 0;
        const int bk = SPH ? best & (int)kPrimMask : best;
        const bool tie = sph ? (none || !bSph || k > bk) : (!none && !bSph && k < bk);
        redo = redo || (t >= closest && t < bestLo);   // not better, but inside the current best's window
        if (t < closest || (t == closest && tie)) {
            bool take = true;
            float lo = -__builtin_inff();
            if (leafBoxes) {
                const SlabHit b = refLeafBox(q, sph, o, inv, tmin, __builtin_inff());
                take = b.hit && !(closest < b.lo);
                redo = redo || (b.hit && closest < b.lo);   // the current best inside this one's window
                lo = t < b.lo ? b.lo : lo;
            }
            if (take) {
                closest = t;
                best = k | (sph ? (int)kSphereBit : 0);
                bestLo = lo;
            }
        }
    }
}

// The same rule decided once per query instead of once per candidate (the non-instanced wide render
// kernels on triangle-only scenes).  The loop keeps the plain minimum M of
// (t, ascending rank) over the candidates and t2, the second-smallest candidate distance (an equal
// t counts): closest <= t2 always, so t2' is the median of (t, closest, t2).  When the query ends,
// deferredRedo tests M's exact box with tmax = inf.
//  - A candidate inside its own box (lo <= t) is tested by the reference whenever it could improve
//    the hit (its ancestors' boxes contain its box and the slab arithmetic is monotone, so they
//    pass too) and is accepted iff t < closest.  If M is one, the reference ends with M: nothing
//    before it holds a smaller or an equal-and-earlier t, nothing after it is closer.
//  - M grazing (t_M < lo_M): the reference tests M iff its closest hit of that moment is >= lo_M,
//    and every hit it can hold is a candidate with t >= t_M.  No other candidate in [t_M, lo_M),
//    which is t2 >= lo_M: M is tested, accepted and final.  Otherwise the query is order-dependent.
//  - A box the ray misses outright: the reference never tests M; order-dependent.
// An order-dependent query is repeated in the reference's order (traceRefStackless), which is
// exact by construction.  The running `closest` that culls nodes is >= t_M, and the wide planes lie
// at least 2^emin outside the exact boxes, far beyond the rounding that opens a window [t, lo): M
// and every candidate inside its window are visited (wideHits).
// q is an edge-form record {v0, rank}{e1, .}{e2, .} (DevScene::wprims of these launches): e1 = v1 -
// v0 and e2 = v2 - v0 are the subtractions primHitAny starts with, done once per triangle when the
// tree is built (pt::edgeTriRecords) -- the same bits, six VALU fewer per test.
//
// Straight-line code: primHitAny's arithmetic in its written order, then its decisions as lane masks
// (ballots of plain compares, scalar logic) and three selects.  hasM: the lanes that test a
// primitive (the others hold record 0 and keep their state).  A candidate is a lane with
//   det != 0  (NaN passes, as `det == 0` does not reject it),
//   none of b1 >= 1, b1 <= 0, b2 >= 1, b2 <= 0, b1 + b2 >= 1  (primHitT's tests and NaN reasoning),
//   t > tmin  (`!(t <= tmin)` and the caller's `t >= 0` in one: tmin > 0, and a NaN fails both forms).
// det == 0 gives inv = +-inf and infinite or NaN t, b1, b2, which no select lets through.
// The reciprocal's IEEE-division fallback (pt_math.hpp rcpRN) is the one branch left, taken by the
// wave when any testing lane needs it.
__device__ __forceinline__ float rcpRNWave(float x, uint64_t hasM) {
    if constexpr (!PT_FAST_RCP) return 1.0f / x;
    const uint32_t ex = (__float_as_uint(x) >> 23) & 0xffu;
    const uint64_t slowM = hasM & __ballot(ex - kRcpExpLo > kRcpExpHi - kRcpExpLo);
    float y = rcpNewton(x);
    if (__builtin_expect(slowM != 0, 0)) y = __builtin_amdgcn_inverse_ballot_w64(slowM) ? 1.0f / x : y;
    return y;
}
// A ray direction's three reciprocals with one range check for the wave (the wide kernels' ray
// start): rcpRN per component costs a compare, an exec save / restore and a branch around the
// division each.  rcpKey moves the biased exponent to the top byte and turns it by 255 - kRcpExpHi,
// so the exponents outside [kRcpExpLo, kRcpExpHi] are the keys below kRcpKeyLim; the smallest of the
// three keys is balloted (among the lanes that run this: the caller's exec mask), and the wave takes
// the IEEE divisions when any lane needs one.  Per lane and component the value is rcpRN's: the
// division exactly where rcpRN divides.
constexpr uint32_t kRcpKeyLim = (255u - kRcpExpHi + kRcpExpLo) << 24;
__device__ __forceinline__ uint32_t rcpKey(float x) { return (__float_as_uint(x) << 1) + ((255u - kRcpExpHi) << 24); }
__device__ __forceinline__ float3 rcpRN3Wave(float3 d) {
    if constexpr (!PT_FAST_RCP) return f3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    const uint32_t kx = rcpKey(d.x), ky = rcpKey(d.y), kz = rcpKey(d.z);
    const uint64_t slowM = __ballot(min(min(kx, ky), kz) < kRcpKeyLim);
    float3 y = f3(rcpNewton(d.x), rcpNewton(d.y), rcpNewton(d.z));
    if (__builtin_expect(slowM != 0, 0)) {
        y.x = kx < kRcpKeyLim ? 1.0f / d.x : y.x;
        y.y = ky < kRcpKeyLim ? 1.0f / d.y : y.y;
        y.z = kz < kRcpKeyLim ? 1.0f / d.z : y.z;
    }
    return y;
}
__device__ __forceinline__ void wideTestTri(const Prim& q, uint64_t hasM, float3 o, float3 d, float tmin, float& closest,
                                            int& best, float& t2) {
    const float3 v0 = xyz(q.p0), e1 = xyz(q.p1), e2 = xyz(q.p2);
    const float3 s1 = cross3(d, e2);
    const float det = dot3(s1, e1);
    const float3 s = sub(o, v0);
    const float3 s2 = cross3(s, e1);
    const float inv = rcpRNWave(det, hasM);
    const float t = dot3(s2, e2) * inv;
    const float b1 = dot3(s1, s) * inv;
    const float b2 = dot3(s2, d) * inv;
    const int k = (int)__float_as_uint(q.p0.w);
    const uint64_t rejM = __ballot(b1 >= 1.0f) | __ballot(b1 <= 0.0f) | __ballot(b2 >= 1.0f) | __ballot(b2 <= 0.0f) |
                          __ballot(b1 + b2 >= 1.0f);
    const uint64_t hitM = hasM & __ballot(det != 0.0f) & __ballot(t > tmin) & ~rejM;
    // the minimum of (t, ascending rank)  (t == closest: a finite hit, best >= 0)
    const uint64_t takeM = hitM & (__ballot(t < closest) | (__ballot(t == closest) & __ballot(k < best)));
    const float mid = __builtin_amdgcn_fmed3f(t, closest, t2);
    t2 = __builtin_amdgcn_inverse_ballot_w64(hitM) ? mid : t2;
    closest = __builtin_amdgcn_inverse_ballot_w64(takeM) ? t : closest;
    best = __builtin_amdgcn_inverse_ballot_w64(takeM) ? k : best;
}
// Is the finished query (closest, t2) order-dependent?  xy, z: the best hit's exact box (DevScene::wbox:
// refLeafBox's planes as {mn, mx} pairs per axis), under refLeafBox's slab arithmetic.
__device__ __forceinline__ bool deferredRedo(float4 xy, float2 z, float3 o, float3 inv, float closest, float t2) {
    const SlabHit b = slabPair(v2f{xy.x, xy.y}, v2f{xy.z, xy.w}, v2f{z.x, z.y}, o, inv, 0.001f, __builtin_inff());
    return !b.hit || (closest < b.lo && t2 < b.lo);
}

// One compressed 8-wide node (five 16-B words, layout in host/pt_wide8.cpp) against the ray:
// returns the hit mask, internal children in bits 24 + (slot ^ oct), leaf primitives in bits
// 0..23 (offsets from the node's primitive base).  Plane distances t = q * (s * inv) + (p - o) *
// inv; the planes lie at least the tree's smallest quantum 2^emin outside the exact boxes (one
// node quantum up to round 6), beyond this arithmetic's rounding,
// and a NaN (0 * inf on an axis the ray is parallel to) only drops that plane: the test never
// rejects a box the exact slab test (aabb.h:21-34) accepts.
//
// The margin holds while |p - o| stays within about 11 times the larger of the scene's extent
// and its coordinates (the margin is >= 2^-18 of that, the rounding of the ray's plane distances
// about 2^-21.6 of |p - o|): a ray whose origin lies farther than 8 scene extents from the
// scene's centre (wideFar) skips this test and is traced in the reference's order instead.
//
// MIX: the plane bytes as fp16 denormals into v_fma_mix_f32 (pt_math.hpp fmaMixLo), the scales
// a = s * inv taken times 2^24 -- the same t bit for bit while |s * 2^24 * inv| stays finite,
// which holds for |inv| <= DevScene::mixLim (a ray with a larger finite |inv| component takes the
// reference-order query instead: mixUnsafe).
// DEC3: the scales decoded in three VALU per axis instead of four -- the exponent byte by v_bfe_u32,
// (byte << 23) + (bias << 23) as one v_lshl_add_u32, the multiply: the same integer into the same
// multiply.  Only where the register it holds longer is free (the sample-mode TRI render kernels;
// DESIGN.md section 11 items 15 B and 16): everywhere else it spills or costs a wave per SIMD.
template <bool MIX = false, bool DEC3 = false>
__device__ __forceinline__ uint32_t wideHits(uint4 n0, uint4 n1, uint4 n2, uint4 n3, uint4 n4, float3 o, float3 inv,
                                             uint32_t oct, float tmin, float tmax) {
    constexpr uint32_t kMixExp = MIX ? 24u : 0u;   // s * 2^24: the exponent byte + 24 (< 255: mixLim's bound)
    float ax, ay, az;
    if constexpr (DEC3) {
        uint32_t ex, ey, ez;   // (in asm: from `(n0.w >> 8) & 0xff` the compiler makes shift, mask, add, multiply)
        asm("v_bfe_u32 %0, %1, 0, 8" : "=v"(ex) : "v"(n0.w));
        asm("v_bfe_u32 %0, %1, 8, 8" : "=v"(ey) : "v"(n0.w));
        asm("v_bfe_u32 %0, %1, 16, 8" : "=v"(ez) : "v"(n0.w));
        ax = __uint_as_float((ex << 23) + (kMixExp << 23)) * inv.x;
        ay = __uint_as_float((ey << 23) + (kMixExp << 23)) * inv.y;
        az = __uint_as_float((ez << 23) + (kMixExp << 23)) * inv.z;
    } else {
        ax = __uint_as_float(((n0.w & 0xffu) + kMixExp) << 23) * inv.x;
        ay = __uint_as_float((((n0.w >> 8) & 0xffu) + kMixExp) << 23) * inv.y;
        az = __uint_as_float((((n0.w >> 16) & 0xffu) + kMixExp) << 23) * inv.z;
    }
    const float bx = (__uint_as_float(n0.x) - o.x) * inv.x;
    const float by = (__uint_as_float(n0.y) - o.y) * inv.y;
    const float bz = (__uint_as_float(n0.z) - o.z) * inv.z;
    // near / far planes per axis: qlo for a positive direction, qhi for a negative one.  The signs
    // are read off inv itself: `oct` is (inv.x < 0) | (inv.y < 0) << 1 | (inv.z < 0) << 2 wherever it
    // is set, in the same statement as inv or right behind it (PT_BEGIN_RAY, wideStart; instanced
    // scenes recompute both on entering an instance whose matrix turns the direction and on leaving
    // it, and keep both otherwise), so these are oct's bits, NaN included (false both ways) -- as
    // compares of values the step holds anyway, not three masks and three integer compares of oct.
    const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
    const uint32_t nearX[2] = {sx ? n2.z : n2.x, sx ? n2.w : n2.y}, farX[2] = {sx ? n2.x : n2.z, sx ? n2.y : n2.w};
    const uint32_t nearY[2] = {sy ? n3.z : n3.x, sy ? n3.w : n3.y}, farY[2] = {sy ? n3.x : n3.z, sy ? n3.y : n3.w};
    const uint32_t nearZ[2] = {sz ? n4.z : n4.x, sz ? n4.w : n4.y}, farZ[2] = {sz ? n4.x : n4.z, sz ? n4.y : n4.w};
    uint32_t hits = 0u;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t meta4 = h ? n1.w : n1.z;
        // per byte: internal children (0b001_11xxx) get their slot bits XOR the ray octant
        // (bits 4 and 3 of the byte, and the mask, in one three-input AND)
        const uint32_t inner4 = __builtin_amdgcn_bitop3_b32(meta4, meta4 << 1, 0x10101010u, 0x80);
        // the octant in the bytes of internal children: 0x01 per such byte times oct (<= 7, no carry
        // between bytes) as one packed 16-bit multiply (pt_math.hpp mulHalves) -- full rate, where the
        // 32-bit v_mul_lo_u32 is quarter rate.  (Every caller passes the bare octant: `oct & 7u` or WideWalk::oct.)
        const uint32_t inner1 = inner4 >> 4;
        const uint32_t bitIndex4 = (meta4 ^ mulHalves(inner1, oct)) & 0x1f1f1f1fu;
        // The counts as a word of their own the compiler cannot trace back to meta4: each child's
        // `byte of childBits4 << byte of bitIndex4` below is then ONE shift with both byte selects
        // (SDWA), where a count taken from meta4 directly is a v_bfe_u32 per child first.
        uint32_t childBits4 = (meta4 >> 5) & 0x07070707u;
        asm("" : "+v"(childBits4));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float tnx, tny, tnz, tfx, tfy, tfz;
            if constexpr (MIX) {   // children j, j ^ 1 share an fp16 pair (the perms are redone per child:
                                   // cheaper in registers than six pairs live across two children)
                const bool hi = (j & 2) != 0;
                const uint32_t px = hi ? planePairHi(nearX[h]) : planePairLo(nearX[h]);
                const uint32_t py = hi ? planePairHi(nearY[h]) : planePairLo(nearY[h]);
                const uint32_t pz = hi ? planePairHi(nearZ[h]) : planePairLo(nearZ[h]);
                const uint32_t qx = hi ? planePairHi(farX[h]) : planePairLo(farX[h]);
                const uint32_t qy = hi ? planePairHi(farY[h]) : planePairLo(farY[h]);
                const uint32_t qz = hi ? planePairHi(farZ[h]) : planePairLo(farZ[h]);
                if (j & 1) {
                    tnx = fmaMixHi(px, ax, bx); tny = fmaMixHi(py, ay, by); tnz = fmaMixHi(pz, az, bz);
                    tfx = fmaMixHi(qx, ax, bx); tfy = fmaMixHi(qy, ay, by); tfz = fmaMixHi(qz, az, bz);
                } else {
                    tnx = fmaMixLo(px, ax, bx); tny = fmaMixLo(py, ay, by); tnz = fmaMixLo(pz, az, bz);
                    tfx = fmaMixLo(qx, ax, bx); tfy = fmaMixLo(qy, ay, by); tfz = fmaMixLo(qz, az, bz);
                }
            } else {
                tnx = __builtin_fmaf((float)((nearX[h] >> (8 * j)) & 0xffu), ax, bx);
                tny = __builtin_fmaf((float)((nearY[h] >> (8 * j)) & 0xffu), ay, by);
                tnz = __builtin_fmaf((float)((nearZ[h] >> (8 * j)) & 0xffu), az, bz);
                tfx = __builtin_fmaf((float)((farX[h] >> (8 * j)) & 0xffu), ax, bx);
                tfy = __builtin_fmaf((float)((farY[h] >> (8 * j)) & 0xffu), ay, by);
                tfz = __builtin_fmaf((float)((farZ[h] >> (8 * j)) & 0xffu), az, bz);
            }
            float lo, hi;
            if (MIX && (j & 1)) {
                lo = max3Raw(max3Raw(tnx, tny, tnz), tmin, tmin);
                hi = min3Raw(min3Raw(tfx, tfy, tfz), tmax, tmax);
            } else {
                lo = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), tmin);
                hi = fminf(fminf(fminf(tfx, tfy), tfz), tmax);
            }
            const uint32_t bits = ((childBits4 >> (8 * j)) & 0xffu) << ((bitIndex4 >> (8 * j)) & 0xffu);
            hits |= lo <= hi ? bits : 0u;
        }
    }
    return hits;
}

// A direction parallel to an axis plane (a component +-0: |1/d| = inf; NaN counts too).
__device__ __forceinline__ bool zeroAxes(float3 inv) {
    return !(fmaxf(fmaxf(fabsf(inv.x), fabsf(inv.y)), fabsf(inv.z)) < __builtin_inff());
}
// One axis the ray is parallel to (d = +-0, 1/d = +-inf), for the 8 children of a wide node: aabb::hit
// (aabb.h:21-34) gives (plane - o) * (1/d) = -inf / +inf by the side of each plane o lies on (NaN when
// on it, which the reference's ternaries skip), so the axis bounds nothing when o lies between a
// child's two planes and rejects the child otherwise.  wideHits' decomposed form q * (s * inv) +
// (p - o) * inv is NaN for every plane of such an axis (never a wrong rejection, never a rejection
// at all: the ray would enter every child it overlaps in the other two axes -- round 4: 1,000-1,500
// node visits for C5 rays at the height of the origin).  Here the test itself, on the quantised
// planes p + q * s: u = (o - p) / s (1 / s a power of two), a child is kept when qlo <= u <= qhi.
// (The rounding of o - p is far below the planes' outward margin of >= 2^emin, as in wideHits.)
// k0 / k1: the children 0-3 / 4-7 byte masks, cleared (bits 5-7) for rejected children.
__device__ __forceinline__ void zeroAxisKeep(float oc, uint32_t pbits, uint32_t ebyte, uint32_t qlo0, uint32_t qlo1,
                                             uint32_t qhi0, uint32_t qhi1, uint32_t& k0, uint32_t& k1) {
    const float u = (oc - __uint_as_float(pbits)) * __uint_as_float((254u - ebyte) << 23);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float l0 = (float)((qlo0 >> (8 * j)) & 0xffu), h0 = (float)((qhi0 >> (8 * j)) & 0xffu);
        const float l1 = (float)((qlo1 >> (8 * j)) & 0xffu), h1 = (float)((qhi1 >> (8 * j)) & 0xffu);
        if (u < l0 || u > h0) k0 &= ~(0xe0u << (8 * j));   // (NaN u: kept)
        if (u < l1 || u > h1) k1 &= ~(0xe0u << (8 * j));
    }
}
// Instanced scenes' node test (they have no reference-order query to hand such rays to): a wave with
// a lane whose ray -- in the current space -- is parallel to an axis plane clears the meta bytes of
// the children that lane's exact slab test rejects on that axis (zeroAxisKeep), then runs the usual
// test.  A wave-uniform branch: the common case pays the ballot only, and no registers stay live.
__device__ __forceinline__ uint32_t wideHitsInst(uint4 n0, uint4 n1, uint4 n2, uint4 n3, uint4 n4, float3 o,
                                                 float3 inv, uint32_t oct, float tmin, float tmax) {
    if (__ballot(zeroAxes(inv)) != 0) {
        const float inf = __builtin_inff();
        uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu;
        if (!(fabsf(inv.x) < inf)) zeroAxisKeep(o.x, n0.x, n0.w & 0xffu, n2.x, n2.y, n2.z, n2.w, k0, k1);
        if (!(fabsf(inv.y) < inf)) zeroAxisKeep(o.y, n0.y, (n0.w >> 8) & 0xffu, n3.x, n3.y, n3.z, n3.w, k0, k1);
        if (!(fabsf(inv.z) < inf)) zeroAxisKeep(o.z, n0.z, (n0.w >> 16) & 0xffu, n4.x, n4.y, n4.z, n4.w, k0, k1);
        n1.z &= k0;
        n1.w &= k1;
    }
    return wideHits<false>(n0, n1, n2, n3, n4, o, inv, oct, tmin, tmax);
}

// The ray origin lies farther than 8 scene extents from the scene's centre on some axis, beyond
// the distance the wide boxes' margin covers (wideHits): the query runs in the reference's order.
constexpr float kWideFarExt = pt::kW8FarExt;   // tied to the builders' quantum in host/pt_wide8.hpp
__device__ __forceinline__ bool wideFar(float cx, float cy, float cz, float ext, float3 o) {
    const float m = fmaxf(fmaxf(fabsf(o.x - cx), fabsf(o.y - cy)), fabsf(o.z - cz));
    return !(m <= kWideFarExt * ext);   // (NaN: far)
}
__device__ __forceinline__ bool wideFar(const DevScene& S, float3 o) { return wideFar(S.cx, S.cy, S.cz, S.ext, o); }
// Instanced scenes draw the line at kInstFarExt = 2 world extents (PT_INST_FAR_EXT, host/pt_render_plan.hpp)
static_assert(kInstFarExt >= 1.0f, "instEntry's cube (centre +- ext) must lie inside the quantised reach");
__device__ __forceinline__ bool instFar(const DevScene& S, float3 o) {
    const float m = fmaxf(fmaxf(fabsf(o.x - S.cx), fabsf(o.y - S.cy)), fabsf(o.z - S.cz));
    return !(m <= kInstFarExt * S.ext);   // (NaN: far)
}

// Instanced scenes have no reference-order query: a ray whose origin lies beyond the region the
// planes' margin covers (instFar) is moved along itself to its entry into the cube centre +- ext
// (ext = the world box's LARGEST extent, so the cube is the world box grown by at least ext / 2 on
// every side) -- no geometry lies before that point, and the new origin lies within 1 extent of the
// centre (max norm), inside the 2-extent reach every instanced tree was quantised for
// (buildInstanced; kInstFarExt >= 1 keeps the cube inside that reach).
// Returns the distance moved (0 when the ray misses that box or starts inside it).
__device__ __forceinline__ float instEntry(float cx, float cy, float cz, float ext, float3& o, float3 d, float3 inv) {
    const float lx = (cx - ext - o.x) * inv.x, hx = (cx + ext - o.x) * inv.x;
    const float ly = (cy - ext - o.y) * inv.y, hy = (cy + ext - o.y) * inv.y;
    const float lz = (cz - ext - o.z) * inv.z, hz = (cz + ext - o.z) * inv.z;
    const float t0 = fmaxf(fmaxf(fminf(lx, hx), fminf(ly, hy)), fminf(lz, hz));
    const float t1 = fminf(fminf(fmaxf(lx, hx), fmaxf(ly, hy)), fmaxf(lz, hz));
    if (!(t0 > 0.0f) || !(t0 <= t1)) return 0.0f;
    o = add(o, scale(t0, d));
    return t0;
}

// A reciprocal direction component larger than `lim` (DevScene::mixLim: a ray nearly parallel to
// an axis plane) would overflow the MIX plane scale s * 2^24 * inv (wideHits); such a ray takes the
// reference-order query.  So does an infinite component (a direction component of exactly 0): the
// decomposed plane distance fma(q, s * inv, (base - o) * inv) is then NaN for most planes, the
// NaN-ignoring min / max drop that axis's bound, and the ray would enter every box it overlaps in
// the other two axes (round 4: 1,000-1,500 node visits for C5 rays at the origin's height against a
// median of 1).  NaN: unsafe.
__device__ __forceinline__ bool mixUnsafe(float3 inv, float lim) {
    const float x = fabsf(inv.x), y = fabsf(inv.y), z = fabsf(inv.z);
    return !(x <= lim) || !(y <= lim) || !(z <= lim);
}

// RenderManager::hitBvh (render_manager.h:86-135): same visiting order (left child, right
// child, leaf children tested at once, internal children pushed left then right).
// Returns the leaf slot of the closest hit or -1; `closest` holds its t.
template <int STACK>
__device__ __forceinline__ int trace(const DevScene& S, float3 o, float3 d, float tmin, float& closest,
                                     uint32_t* stk, Counters& c) {
    int best = -1;
    if (S.nprims <= 0) return -1;
    if (S.nprims == 1) {   // root is a leaf: tested without a box test (:92-98)
        const uint32_t ref = kLeafBit | (__float_as_uint(S.prims[2].w) ? kSphereBit : 0u);
        primTest(S, ref, o, d, tmin, closest, best, c);
        return best;
    }
    const float3 inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));
    int node = 0, sp = 0, guard = 0;
    for (;;) {
        // Each internal node is visited at most once per query; more means a corrupt tree.
        if (++guard > S.nprims) { atomicOr(S.err, 1u); break; }
        c.visits++;
        const float4* np = S.nodes + 4 * (size_t)node;
        const float4 a = np[0], b = np[1], q = np[2], r = np[3];
        const uint32_t lref = __float_as_uint(r.x), rref = __float_as_uint(r.y);
        if (slabLeft(a, b, o, inv, tmin, closest).hit) {
            if (lref & kLeafBit) primTest(S, lref, o, d, tmin, closest, best, c);
            else if (sp < STACK) { stk[sp * kWave] = lref; sp++; }
            else { atomicOr(S.err, 2u); break; }
        }
        if (slabRight(b, q, o, inv, tmin, closest).hit) {
            if (rref & kLeafBit) primTest(S, rref, o, d, tmin, closest, best, c);
            else if (sp < STACK) { stk[sp * kWave] = rref; sp++; }
            else { atomicOr(S.err, 2u); break; }
        }
        if (sp == 0) break;
        sp--;
        node = (int)stk[sp * kWave];
    }
    return best;
}

// RenderManager::hitBvh (render_manager.h:86-135) without a stack, for the wide kernels' rare
// order-dependent queries: the same primitive tests in the same order with the same `closest`.
// The reference pushes an internal child when its box passes at the parent's visit and pops
// right before left; here a child is entered when its box passes at the moment it would be
// popped (parent links lead back up).  A box that passed earlier but fails now has children
// that all fail now (their boxes are inside it; correctly rounded slab arithmetic is monotonic),
// so skipping it changes no primitive test.  Returns the leaf k of the closest hit or -1.
__device__ __forceinline__ int traceRefStackless(const DevScene& S, float3 o, float3 d, float tmin, float& closest) {
    int best = -1;
    if (S.nprims <= 0) return -1;
    if (S.nprims == 1) {   // root is a leaf: tested without a box test (:92-98)
        const float t1 = primHitT(loadPrim(S, 0), __float_as_uint(S.prims[2].w) != 0, o, d, tmin, closest);
        if (t1 >= 0.0f) { closest = t1; best = 0; }
        return best;
    }
    const float3 inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));
    int node = 0, from = -1;   // from >= 0: returning from that child of `node`
    bool finished = false;
    for (int guard = 0; guard <= 4 * S.nprims; guard++) {   // each node is entered and left once
        const float4* np = S.nodes + 4 * (size_t)node;
        const float4 a = np[0], b = np[1], q = np[2], r = np[3];
        const uint32_t lref = __float_as_uint(r.x), rref = __float_as_uint(r.y);
        int next = -1;
        if (from < 0) {   // visit: the leaf children in order, then the right subtree, then the left
            const SlabHit hl = slabLeft(a, b, o, inv, tmin, closest);
            if (hl.hit && (lref & kLeafBit)) {
                const float t = primHitT(loadPrim(S, lref & kPrimMask), (lref & kSphereBit) != 0, o, d, tmin, closest);
                if (t >= 0.0f) { closest = t; best = (int)(lref & kPrimMask); }
            }
            const SlabHit hr = slabRight(b, q, o, inv, tmin, closest);
            if (hr.hit && (rref & kLeafBit)) {
                const float t = primHitT(loadPrim(S, rref & kPrimMask), (rref & kSphereBit) != 0, o, d, tmin, closest);
                if (t >= 0.0f) { closest = t; best = (int)(rref & kPrimMask); }
            }
            if (hr.hit && !(rref & kLeafBit)) next = (int)rref;
            else if (!(lref & kLeafBit) && slabLeft(a, b, o, inv, tmin, closest).hit) next = (int)lref;
        } else if ((uint32_t)from == rref && !(lref & kLeafBit) && slabLeft(a, b, o, inv, tmin, closest).hit) {
            next = (int)lref;
        }
        if (next >= 0) {
            node = next;
            from = -1;
        } else {
            if (node == 0) { finished = true; break; }
            from = node;
            node = S.iparent[node];
        }
    }
    if (!finished) atomicOr(S.err, 4u);   // a corrupt tree or parent links: reported, never silent
    return best;
}

// Hit record for leaf slot k at distance t (cuda_object.h:62-67 / 85-88, hit_record.h:21-24),
// with the hit object's material (material.h:17-68) carried along: the three independent 16-B
// loads of the shading record are one memory round trip (instead of prim -> normal -> material).
struct HitRec { float3 p, n; int mat, obj; bool front; float4 m0; float ir; int type; };

// SPH = false: no record is a sphere (the TRI kernels), so the sphere normal is not compiled in.
// The record's address is a 32-bit byte offset off the uniform base (48 k < 2^32: k < 2^26,
// pt_scene_create), like the LEAF step's primitive records: no 64-bit multiply.
template <bool SPH = true>
__device__ __forceinline__ HitRec makeHitFrom(const float4* shade, int k, float t, float3 o, float3 d) {
    HitRec h;
    const float4* r = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(shade) + mul48((uint32_t)k));
    const float4 s0 = r[0], s1 = r[1], s2 = r[2];
    const uint32_t tf = __float_as_uint(s2.y);
    h.p = add(o, scale(t, d));
    float3 outward = xyz(s0);
    if constexpr (SPH) {
        if (tf >> 16) outward = divs(sub(h.p, xyz(s0)), s0.w);   // sphere: (p - c) / r
    }
    h.front = dot3(d, outward) < 0.0f;
    h.n = h.front ? outward : neg(outward);
    h.mat = (int)__float_as_uint(s2.z);
    h.obj = (int)__float_as_uint(s2.w);
    h.m0 = s1;
    h.ir = s2.x;
    h.type = (int)(tf & 0xffffu);
    return h;
}
__device__ __forceinline__ HitRec makeHit(const DevScene& S, int k, float t, float3 o, float3 d) {
    return makeHitFrom(S.shade, k, t, o, d);
}

// Instanced scenes: the world ray (o, d) entering an instance, in its object space (rows r0..r2 of
// the world-to-object transform; the hit distance t is the same parameter in both spaces).
__device__ __forceinline__ float3 xformPoint(float4 r0, float4 r1, float4 r2, float3 p) {
    return f3(((r0.x * p.x + r0.y * p.y) + r0.z * p.z) + r0.w, ((r1.x * p.x + r1.y * p.y) + r1.z * p.z) + r1.w,
              ((r2.x * p.x + r2.y * p.y) + r2.z * p.z) + r2.w);
}
__device__ __forceinline__ float3 xformDir(float4 r0, float4 r1, float4 r2, float3 v) {
    return f3((r0.x * v.x + r0.y * v.y) + r0.z * v.z, (r1.x * v.x + r1.y * v.y) + r1.z * v.z,
              (r2.x * v.x + r2.y * v.y) + r2.z * v.z);
}
// Hit record of instance key `key` (instance << gBits | shading index) at distance t of the world
// ray: the object-space shading record, the outward normal returned to the world by the inverse
// transpose and normalised (cuda_object.h:62-67 / 85-88 in object space, hit_record.h:21-24 in the
// world); an instance whose linear part is the identity (a translation) keeps the record's normal as
// is, the flattened scene's arithmetic.
__device__ __forceinline__ HitRec makeHitInst(const DevScene& S, uint32_t key, float t, float3 o, float3 d, int& obj) {
    const uint32_t inst = key >> S.gBits, g = key & ((1u << S.gBits) - 1u);
    const float4* ir = S.winst + 4 * (size_t)inst;
    const float4 r0 = ir[0], r1 = ir[1], r2 = ir[2], ex = ir[3];
    const float4* r = S.wshade + 3 * (size_t)g;
    const float4 s0 = r[0], s1 = r[1], s2 = r[2];
    const uint32_t tf = __float_as_uint(s2.y);
    const bool ident = __float_as_uint(ex.y) == 1u, linIdent = __float_as_uint(ex.y) != 0u;
    HitRec h;
    h.p = add(o, scale(t, d));
    float3 outward;
    if (tf >> 16) {   // sphere: (p - c) / r in object space
        const float3 po = ident ? h.p : xformPoint(r0, r1, r2, h.p);
        outward = divs(sub(po, xyz(s0)), s0.w);
    } else {
        outward = xyz(s0);
    }
    if (!linIdent) {   // n_world = normalize(A^-T n_object): A^-1's columns dotted with n
        const float3 n = outward;
        outward = normalize3(f3((r0.x * n.x + r1.x * n.y) + r2.x * n.z, (r0.y * n.x + r1.y * n.y) + r2.y * n.z,
                                (r0.z * n.x + r1.z * n.y) + r2.z * n.z));
    }
    h.front = dot3(d, outward) < 0.0f;
    h.n = h.front ? outward : neg(outward);
    h.mat = (int)__float_as_uint(s2.z);
    obj = (int)(__float_as_uint(ex.x) + __float_as_uint(s2.w));   // the object's index in the flattened order
    h.obj = obj;
    h.m0 = s1;
    h.ir = s2.x;
    h.type = (int)(tf & 0xffffu);
    return h;
}

// ------------------------------------------------------------------------ BSDFs
// utility.h:51-62 / 73-82; vec3(...) arguments drawn x, y, z in order.
// (trials: PT_DIAG builds count the lane's trials there; unused otherwise)
template <class G>
__device__ __forceinline__ float3 onUnitSphere(G& g, uint32_t* trials = nullptr) {
    float3 res;
    float norm;
    (void)trials;
    do {   // draws x, y, z in order; centered2() = 2 * (uniform() - 0.5f) exactly
        res = g.centered2x3();
        norm = len2(res);
#ifdef PT_DIAG
        if (trials) ++*trials;
#endif
    } while (norm >= 1.0f);
    return divs(res, sqrtf(norm));
}
template <class G>
__device__ __forceinline__ float3 inUnitSphere(G& g) {
    float3 res;
    do {
        res = g.centered2x3();
    } while (len2(res) >= 1.0f);
    return res;
}
__device__ __forceinline__ float3 reflect3(float3 v, float3 n) { return sub(v, scale(2.0f * dot3(v, n), n)); }

// Material::scatter (material.h:28-61); returns false when the path is absorbed.
template <class G>
__device__ __forceinline__ bool scatter(const DevScene& S, const HitRec& h, float3& d, float3& atten, G& g) {
    (void)S;
    const float4 m0 = h.m0;
    const int type = h.type;
    if (type == PT_LAMBERTIAN) {
        float3 dir = add(h.n, onUnitSphere(g));
        if (fabsf(dir.x) < 1e-7f && fabsf(dir.y) < 1e-7f && fabsf(dir.z) < 1e-7f) dir = h.n;
        d = dir;
        atten = xyz(m0);
        return true;
    }
    if (type == PT_METAL) {
        float3 refl = reflect3(normalize3(d), h.n);
        float3 fz = inUnitSphere(g);
        d = add(refl, scale(m0.w, fz));
        atten = xyz(m0);
        return dot3(d, h.n) > 0.0f;
    }
    if (type == PT_DIELECTRIC) {
        atten = f3(1.0f, 1.0f, 1.0f);
        const float ir = h.ir;
        float ratio = h.front ? rcpRN(ir) : ir;
        float3 ud = normalize3(d);
        float cos_t = fminf(dot3(neg(ud), h.n), 1.0f);
        float sin_t = sqrtf(1.0f - cos_t * cos_t);
        bool cannot = ratio * sin_t > 1.0f;
        bool refl = cannot;
        if (!cannot) {   // reflectance (physical.h:20-25), pow(x,5) = ((x*x)*(x*x))*x
            float r0 = (1.0f - ratio) / (1.0f + ratio);
            r0 = r0 * r0;
            float x = 1.0f - cos_t;
            float x2 = x * x;
            float rf = r0 + (1.0f - r0) * ((x2 * x2) * x);
            refl = rf > g.uniform();
        }
        if (refl) {
            d = reflect3(ud, h.n);
        } else {   // refract (physical.h:14-19)
            float ct = fminf(dot3(neg(ud), h.n), 1.0f);
            float3 perp = scale(ratio, add(ud, scale(ct, h.n)));
            float3 par = scale(-sqrtf(fabsf(1.0f - len2(perp))), h.n);
            d = add(perp, par);
        }
        return true;
    }
    return false;
}

// scatter() with the attenuation applied in place (att *= albedo for Lambertian and metal): the
// dielectric's (1, 1, 1) is skipped, exactly (x * 1.0f == x for the finite attenuations of a
// path), and no attenuation value has to live across the material switch.
template <class G>
__device__ __forceinline__ bool scatterInto(const HitRec& h, float3& d, float3& att, G& g, uint32_t* trials = nullptr) {
    const float4 m0 = h.m0;
    const int type = h.type;
    if (type == PT_LAMBERTIAN) {
        float3 dir = add(h.n, onUnitSphere(g, trials));
        if (fabsf(dir.x) < 1e-7f && fabsf(dir.y) < 1e-7f && fabsf(dir.z) < 1e-7f) dir = h.n;
        d = dir;
        att = mul(att, xyz(m0));
        return true;
    }
    if (type == PT_METAL) {
        float3 refl = reflect3(normalize3(d), h.n);
        float3 fz = inUnitSphere(g);
        d = add(refl, scale(m0.w, fz));
        att = mul(att, xyz(m0));
        return dot3(d, h.n) > 0.0f;
    }
    if (type == PT_DIELECTRIC) {
        const float ir = h.ir;
        float ratio = h.front ? rcpRN(ir) : ir;
        float3 ud = normalize3(d);
        float cos_t = fminf(dot3(neg(ud), h.n), 1.0f);
        float sin_t = sqrtf(1.0f - cos_t * cos_t);
        bool cannot = ratio * sin_t > 1.0f;
        bool refl = cannot;
        if (!cannot) {   // reflectance (physical.h:20-25), pow(x,5) = ((x*x)*(x*x))*x
            float r0 = (1.0f - ratio) / (1.0f + ratio);
            r0 = r0 * r0;
            float x = 1.0f - cos_t;
            float x2 = x * x;
            float rf = r0 + (1.0f - r0) * ((x2 * x2) * x);
            refl = rf > g.uniform();
        }
        if (refl) {
            d = reflect3(ud, h.n);
        } else {   // refract (physical.h:14-19)
            float ct = fminf(dot3(neg(ud), h.n), 1.0f);
            float3 perp = scale(ratio, add(ud, scale(ct, h.n)));
            float3 par = scale(-sqrtf(fabsf(1.0f - len2(perp))), h.n);
            d = add(perp, par);
        }
        return true;
    }
    return false;
}

// Sky (main.cu:34-36) times attenuation.
__device__ __forceinline__ float3 sky(float3 d, float3 att) {
    float3 ud = normalize3(d);
    float t = 0.5f * (ud.y + 1.0f);
    float3 c = add(scale(1.0f - t, f3(1.0f, 1.0f, 1.0f)), scale(t, f3(0.5f, 0.7f, 1.0f)));
    return mul(c, att);
}
// The same between a scene's own horizon H and zenith Z colours (pt_scene_set_sky; wave-uniform,
// from the kernel arguments), in the same operation order: H = (1, 1, 1), Z = (0.5, 0.7, 1) give the
// bits of the function above.
__device__ __forceinline__ float3 sky(float3 d, float3 att, float3 H, float3 Z) {
    float3 ud = normalize3(d);
    float t = 0.5f * (ud.y + 1.0f);
    float3 c = add(scale(1.0f - t, H), scale(t, Z));
    return mul(c, att);
}
// An emissive surface (PT_EMISSIVE: radiance E in the albedo slot of the shading record) ends the
// path with att * E; no draw.  Beside the absorb exit of scatter / scatterInto, which every
// material type other than 1, 2 and 4 takes.
__device__ __forceinline__ float3 emitted(const HitRec& h, float3 att) {
    return h.type == PT_EMISSIVE ? mul(att, xyz(h.m0)) : f3(0.0f, 0.0f, 0.0f);
}
// Next-event estimation (PT_RENDER_NEE, pt.h states the rule and this operation order): the light
// sample of a Lambertian hit at p with normal n; att = the path's attenuation after the hit (the
// attenuation before it times the albedo).  Draws uL, ua, ub whatever follows.  true: the shadow ray
// (p, w) is to be traced, and `term` is what an unoccluded sample adds to the path.
// MIS (PT_RENDER_MIS, pt.h): `term` carries the balance-heuristic weight wl in G's place.
constexpr float kShadowTmax = 0.999f;   // the light sits at t = 1 of the unnormalised shadow ray
constexpr float kPi = 3.1415927f;
// The light sample's pdf per solid angle of the direction of v (unnormalised, from the shaded point to
// the light's plane): d2 = dot(v, v), cl = |dot(cross(e1, e2), v)|.
__device__ __forceinline__ float lightPdf(float nLf, float d2, float cl) {
    return ((2.0f * d2) * sqrtf(d2)) / (nLf * cl);   // (IEEE division and square root)
}
template <bool MIS = false, class G>
__device__ __forceinline__ bool lightSample(const float4* __restrict__ lights, int nL, float3 p, float3 n, float3 att,
                                            G& g, float3& w, float3& term) {
    const float uL = g.uniform();
    float ua = g.uniform(), ub = g.uniform();
    const float nLf = (float)nL;
    const int k = min((int)(uL * nLf), nL - 1);
    if (ua + ub > 1.0f) { ua = 1.0f - ua; ub = 1.0f - ub; }
    ub = fminf(ub, 1.0f - ua);   // (a sum that rounding left an ulp beyond 1: back onto the edge)
    ua = fminf(ua, 1.0f - ub);
    const float4* L = lights + 4 * (size_t)k;
    const float3 v0 = xyz(L[0]), e1 = xyz(L[1]), e2 = xyz(L[2]), E = xyz(L[3]);
    const float3 q = add(add(v0, scale(ua, e1)), scale(ub, e2));
    w = sub(q, p);
    const float cs = dot3(n, w);
    const float cl = fabsf(dot3(cross3(e1, e2), w));
    const float d2 = dot3(w, w);
    term = f3(0.0f, 0.0f, 0.0f);
    if (cs <= 0.0f || cl == 0.0f || d2 == 0.0f) return false;
    float G_;
    if constexpr (MIS) {   // wl = pb / (pl + pb): the scatter's pdf of this direction over the two pdfs' sum
        const float pl = lightPdf(nLf, d2, cl);
        const float pb = cs / (kPi * sqrtf(d2));
        G_ = pb / (pl + pb);
    } else {
        G_ = ((cs * cl) * nLf) / (6.2831855f * (d2 * d2));   // (IEEE division)
    }
    const float3 t = scale(G_, mul(att, E));
    term = f3(t.x != t.x ? 0.0f : t.x, t.y != t.y ? 0.0f : t.y, t.z != t.z ? 0.0f : t.z);
    return true;
}
// The hit on shading record k is a sampled light: an emissive triangle (not an emissive sphere).
__device__ __forceinline__ bool sampledLight(const float4* shade, int k, const HitRec& h) {
    return h.type == PT_EMISSIVE && (__float_as_uint(shade[3 * (size_t)k + 2].y) >> 16) == 0u;
}
// PT_RENDER_MIS: the Lambertian scatter's pdf per solid angle of its own ray's direction d (unnormalised),
// taken at the hit where the rule applies ...
__device__ __forceinline__ float scatterPdf(float3 n, float3 d) {
    return fmaxf(dot3(n, d), 0.0f) / (kPi * sqrtf(dot3(d, d)));
}
// ... and the ending term of that ray when it lands on the sampled light `obj` (object index; slot[obj] =
// its light record) at parameter t: att * E weighted with wb = pbs / (pls + pbs), pls = the light
// sample's pdf of the same direction, from the hit's own t * d.
__device__ __forceinline__ float3 emittedWeightedAt(const float4* __restrict__ lights, uint32_t rec, int nL, float t, float3 d,
                                                    float pbs, float3 attE) {
    const float4* L = lights + 4 * (size_t)rec;
    const float3 e1 = xyz(L[1]), e2 = xyz(L[2]);
    const float3 wv = scale(t, d);
    const float D2 = dot3(wv, wv);
    const float clh = fabsf(dot3(cross3(e1, e2), wv));
    const float wb = pbs / (lightPdf((float)nL, D2, clh) + pbs);
    const float3 c = scale(wb, attE);
    return f3(c.x != c.x ? 0.0f : c.x, c.y != c.y ? 0.0f : c.y, c.z != c.z ? 0.0f : c.z);
}
__device__ __forceinline__ float3 emittedWeighted(const float4* __restrict__ lights, const uint32_t* __restrict__ slot,
                                                  int nL, int obj, float t, float3 d, float pbs, float3 attE) {
    return emittedWeightedAt(lights, slot[obj], nL, t, d, pbs, attE);
}
// An instanced scene's record of hit key `key` (instance << gBits | shading index): the instance's first
// record plus the rank of the object among its mesh's sampled lights (instLightKernel's order).
__device__ __forceinline__ uint32_t instLightSlot(const uint32_t* __restrict__ instFirst, const uint32_t* __restrict__ rank,
                                                  uint32_t key, int gBits) {
    return instFirst[key >> gBits] + rank[key & ((1u << gBits) - 1u)];
}
// A finished sample under NEE: the direct terms plus the path's ending term, clamped per channel.
__device__ __forceinline__ float3 neeTotal(float3 direct, float3 contrib) {
    const float3 t = add(direct, contrib);
    return f3(fminf(t.x, PT_MAX_RADIANCE), fminf(t.y, PT_MAX_RADIANCE), fminf(t.z, PT_MAX_RADIANCE));
}
template <bool NEE>
__device__ __forceinline__ float3 endOf(float3 direct, float3 contrib) {
    if constexpr (NEE) return neeTotal(direct, contrib);
    else return contrib;
}

// ------------------------------------------------------------------------ kernels
struct RenderParams {
    DevScene S;
    DevCamera cam;
    uint32_t *sd, *s0, *s1, *s2, *s3, *s4;   // film RNG state, SoA over local pixels
    float* out;
    unsigned long long* counters;             // rays, visits, tris, spheres, paths
    int width, nrows, stripe_h, nparts, part;
    int tiles_x, ntiles;
    int spp, max_depth;
    float invW, invH, invSpp;
    int leafBatch, shadeBatch;                // wavefront scheduler thresholds (lanes)
    int nodeMin;                              // compat: below this many NODE lanes, run the larger of LEAF / SHADE
    int kernel;                               // PT_KERNEL_*
    unsigned long long* waveTimes;            // optional (PT_WAVE_TIMES): {start, end, tile|xcc<<32} per wave
    const int* tileOrder;                     // launch order of tiles (longest first), or null = identity
    const uint32_t* tileXY;                   // sample mode: tile of each launch slot as tx | ty << 16 (the order decoded)
    int nblocksShift;                         // sample mode: log2(ngroups) when a power of two, else -1
    unsigned* tileCost;                       // out: per-tile wave duration (s_memrealtime ticks, 100 MHz)
    int prioTiles;                            // the first prioTiles tiles of the order run at s_setprio prioLevel
    int prioLevel;                            // 1-3 (s_setprio's user priority; added to the wave's age in issue arbitration)
    // sample mode (RNG_SAMPLE): samples are summed in fixed blocks of `block` samples.  Each
    // (pixel, block) is one task, summed in sample order (fp32) by whichever lane takes it; the
    // block sum is then added to the pixel's accumulator as a 32.32 fixed-point integer
    // (blockFixed), with atomics: integer addition is exact and order-free, so the image does
    // not depend on scheduling or on the stripe partition.  pixAcc[4 * pixel] = {x, y, z, rays}.
    int nblocks, block;
    // A task is one summation block: `span` = block samples, `ngroups` = nblocks tasks per pixel
    // (`group` = 1; the field only keeps the layout).
    int group, span, ngroups;
    unsigned long long* pixAcc;
    unsigned* taskCounter;                    // next task (zeroed before the launch)
    uint32_t* stackSpill;                     // sample mode, STACK > 32: stack entries >= 32 (per wave slot, lane)
    uint32_t ntasks;                          // tile slots x ngroups x 64
    int nwaves;                               // persistent waves launched
    uint32_t seed0, seed1;
    uint32_t sampleBase;                      // sample mode: index of the frame's first sample
    int measureCost;                          // sample mode: count rays per pixel for the tile order
    int camFar;                               // wide: the camera lies beyond the wide boxes' margin (wideFar)
    int rawOut;                               // compat: store the raw sample sum (resolveKernel follows)
    int stripeShift, blockShift;              // log2(stripe_h), log2(block) when powers of two, else -1 (blockShift: no reader left)
    int splitTiles, splitWays;                // compat: the longest tiles run as splitWays waves each
    int compatGrid;                           // compat (tile waves): critWaves + ntiles + splitTiles * (splitWays - 1)
    // compat, critical pixels (wide kernel): the nCrit pixels of critList (the previous launch's
    // longest chains) run first, critLanes per wave (blocks 0 .. critWaves - 1), each lane taking its
    // pixel's whole chain with a per-lane closest-hit traversal inside the ray start (no NODE / LEAF
    // steps); tile waves skip the pixels critFlag marks.  pixRays (optional): rays per pixel.
    int nCrit, critLanes, critWaves;
    const uint32_t* critList;
    const uint8_t* critFlag;
    uint32_t* pixRays;
    // Lit scenes (`lit`: an emissive material or a sky other than the reference's; the kernels' LIT
    // instantiations -- every other scene runs the kernels without either, as before): the scene's
    // sky at enqueue time (pt_scene_set_sky), by value.
    float3 skyH, skyZ;
    int lit;
    // PT_RENDER_NEE (pt.h) on a scene with sampled lights: the light records {v0}{e1}{e2}{E} of the
    // last build and their count nL > 0 (the kernels' NEE instantiations); 0: the rule is off.
    const float4* lights;
    int nLights;
    // PT_RENDER_MIS (with nLights > 0; the kernels' MIS instantiations): object index -> slot in
    // `lights` (the build's scan; read for hits on sampled lights only), and the flag.
    int mis;
    const uint32_t* lightSlot;
    // Instanced scenes built with PT_BVH_LIGHTS: lightSlot is indexed by shading index and holds the
    // object's rank among its mesh's sampled lights; instLightFirst: the first record of each instance.
    const uint32_t* instLightFirst;
    // Flat wide launches: the kernels' TRI instantiations (a triangle-only scene whose edge-form
    // records S.wprims holds, and PT_WIDE_TRI not 0).  Read by the launchers, not by the kernels.
    int tri;
    // Flat wide sample launches without NEE: the kernels' AHEAD instantiations (with tri; no metal or
    // dielectric material, a pinhole camera, a stack of 8 or 16, and PT_SHADE_AHEAD not 0).  Read by
    // the launchers, not by the kernels.
    int ahead;
};
template <bool LIT>
__device__ __forceinline__ float3 skyOf(const RenderParams& P, float3 d, float3 att) {
    if constexpr (LIT) return sky(d, att, P.skyH, P.skyZ);
    else return sky(d, att);
}

// (compat critical pixels -- PT_CRIT_PIXELS, PT_CRIT_LANES, critFor: host/pt_render_plan.hpp)
// (blockFixed, blockFixedSmall, fixedToFloat: pt_math.hpp)
// One finished (pixel, block) task: its sum added to the pixel's accumulator, and -- on frames
// that measure tile costs (`cost`: the input of the next launches' longest-first order) -- its ray
// count; no-return atomics (device scope: 4 of them per task cost 5 % of a C3 frame, so the ray
// counts are taken on one frame in eight).
__device__ __forceinline__ void addBlock(unsigned long long* acc, float3 sum, uint32_t rays, bool cost) {
    // the common case -- every finishing lane's three sums in [0, 2^24), NaN excluded by the >= 0
    // tests -- takes blockFixedSmall (a wave-uniform branch on the ballot)
    const bool small = sum.x >= 0.0f && sum.y >= 0.0f && sum.z >= 0.0f &&
                       fmaxf(fmaxf(sum.x, sum.y), sum.z) < 16777216.0f;
    unsigned long long fx, fy, fz;
    if (__ballot(!small) == 0) {
        fx = blockFixedSmall(sum.x); fy = blockFixedSmall(sum.y); fz = blockFixedSmall(sum.z);
    } else {
        fx = blockFixed(sum.x); fy = blockFixed(sum.y); fz = blockFixed(sum.z);
    }
    __hip_atomic_fetch_add(acc + 0, fx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(acc + 1, fy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(acc + 2, fz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cost) __hip_atomic_fetch_add(acc + 3, (unsigned long long)rays, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Compat mode end of a pixel: sqrt(sum / spp) (main.cu:290-293), or the raw sum when a resolve
// pass (accumulation / 8-bit output) follows.
__device__ __forceinline__ void storePixel(const RenderParams& P, size_t idx, float3 sum) {
    float* outp = P.out + 3 * idx;
    if (P.rawOut) {
        outp[0] = sum.x; outp[1] = sum.y; outp[2] = sum.z;
    } else {
        outp[0] = sqrtf(sum.x * P.invSpp);
        outp[1] = sqrtf(sum.y * P.invSpp);
        outp[2] = sqrtf(sum.z * P.invSpp);
    }
}

// shift: log2(sh) when sh is a power of two, else -1 (shifts instead of two VALU divisions)
__device__ __forceinline__ int globalRowFast(int lrow, int sh, int shift, int nparts, int part) {
    if (nparts == 1) return lrow;
    if (shift >= 0) return ((((lrow >> shift) * nparts + part)) << shift) + (lrow & (sh - 1));
    return ((lrow / sh) * nparts + part) * sh + lrow % sh;
}
__device__ __forceinline__ int globalRow(int lrow, int sh, int nparts, int part) {
    return ((lrow / sh) * nparts + part) * sh + lrow % sh;
}

// Tile scheduling.  Workgroups are dispatched in blockIdx order and dealt round-robin over the 8
// XCDs, so consecutive tiles land on different XCDs (balanced; the C3 BVH fits every L2).  When
// the film has measured per-tile costs from a previous launch, tiles are launched longest first
// (LPT): a tile's 1024 samples per pixel are sequential (per-pixel RNG stream), so the most
// expensive tiles are the critical path and must start first.  Scheduling never changes results.
__device__ __forceinline__ int tileOf(const RenderParams& P, int bid) {
    return P.tileOrder ? P.tileOrder[bid] : bid;
}

__device__ __forceinline__ void waveReduceAdd(unsigned long long* dst, uint32_t v) {
    unsigned long long x = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && x) atomicAdd(dst, x);
}

// SAMPLE: the sample-mode streams and block sums, one wave per tile, samples in order -- the
// same frame as renderKernelWF<STACK, true>, in the reference's traversal order (the bench
// counts algorithmic bytes with it).
// Lens sample of camera::get_ray (camera.h:58-62): a uniform point of the unit disk scaled by the
// lens radius, offset along right / up.  The reference draws it in polar form (utility.h:98-102:
// sqrtf, cosf, sinf) from the SHARED state randState[0] (main.cu:286, raced by every thread), so
// its lens samples are not reproducible; here they come from the path's own stream, right after
// the pixel jitter, by rejection (x, y in [-1, 1) until x^2 + y^2 < 1: the same uniform disk, and
// no transcendental, so the oracle's arithmetic is the kernel's bit for bit).
template <class G>
__device__ __forceinline__ void lensOffset(float3 right, float3 up, float lens, G& g, float3& o, float3& d) {
    float x, y;
    do {
        x = 2.0f * (g.uniform() - 0.5f);
        y = 2.0f * (g.uniform() - 0.5f);
    } while (x * x + y * y >= 1.0f);
    const float rx = lens * x, ry = lens * y;
    const float3 off = add(scale(rx, right), scale(ry, up));
    o = add(o, off);
    d = sub(d, off);
}

// NEE (with LIT): next-event estimation as a nested query -- the shadow ray is traced where the
// Lambertian hit is shaded, then the loop goes on with the scatter ray.
// MIS (with NEE): the light sample's and the scatter ray's weights (PT_RENDER_MIS, pt.h).
template <int STACK, bool SAMPLE, bool LIT = false, bool NEE = false, bool MIS = false>
__global__ __launch_bounds__(kWave) void renderKernel(RenderParams P) {
    static_assert(!MIS || NEE, "MIS: the NEE instantiations only");
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    const int tile = tileOf(P, blockIdx.x);
    const unsigned long long tStart = __builtin_amdgcn_s_memrealtime();
    const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
    const int col = tx * 8 + (lane & 7);
    const int lrow = ty * 8 + (lane >> 3);
    const bool valid = col < P.width && lrow < P.nrows;
    Counters c{0, 0, 0, 0};
    uint32_t paths = 0;
    if (valid) {
        const size_t idx = (size_t)lrow * P.width + col;
        const int row = globalRow(lrow, P.stripe_h, P.nparts, P.part);
        Xorwow g{};
        if constexpr (!SAMPLE) g = Xorwow{P.sd[idx], P.s0[idx], P.s1[idx], P.s2[idx], P.s3[idx], P.s4[idx]};
        const uint32_t gpix = (uint32_t)row * (uint32_t)P.width + (uint32_t)col;
        const float fcol = (float)col, frow = (float)row;
        float3 sum = f3(0.0f, 0.0f, 0.0f);
        float3 o, d, att;
        int depthLeft = 0, sample = 0;
        float3 direct = f3(0.0f, 0.0f, 0.0f);   // NEE: the path's direct terms so far
        bool fromNee = false;                    // NEE: the current ray left a hit where the rule applied
        float pbs = 0.0f;                        // MIS: that ray's scatter pdf
        // newPath: main.cu:284-286 + camera::get_ray (camera.h:58-64): the lens sample from the
        // path's stream (lensOffset), the time draw skipped (no moving objects on the path).
        auto newPath = [&]() {
            if constexpr (SAMPLE) g = sampleStream(P.seed0, P.seed1, P.sampleBase + (uint32_t)sample, gpix);
            float u = (fcol + g.uniform()) * P.invW;
            float v = (frow + g.uniform()) * P.invH;
            o = P.cam.pos;
            d = sub(add(add(P.cam.ll, scale(u, P.cam.hor)), scale(v, P.cam.ver)), P.cam.pos);
            if (P.cam.lens != 0.0f) lensOffset(P.cam.right, P.cam.up, P.cam.lens, g, o, d);
            att = f3(1.0f, 1.0f, 1.0f);
            depthLeft = P.max_depth;
            paths++;
            if constexpr (NEE) { direct = f3(0.0f, 0.0f, 0.0f); fromNee = false; }
        };
        // sample mode: close summation block `b` after its last sample (its sum and its ray count,
        // the tile-cost input of the next launch's longest-first order)
        uint32_t blockRays0 = 0;
        auto flush = [&]() {
            if constexpr (SAMPLE) {
                if (sample % P.block == 0 || sample == P.spp) {
                    addBlock(P.pixAcc + 4 * idx, sum, c.rays - blockRays0 + 1u, P.measureCost != 0);
                    blockRays0 = c.rays;
                    sum = f3(0.0f, 0.0f, 0.0f);
                }
            }
        };
        if (P.max_depth <= 0) {
            while (sample < P.spp) {
                newPath();
                const float3 c0 = skyOf<LIT>(P, d, att);
                sum = add(sum, NEE ? neeTotal(direct, c0) : c0);
                sample++;
                flush();
            }
        } else if (P.spp > 0) {
            newPath();
            uint32_t* my = stk + lane;
            for (;;) {
                // one bounce of rayTracing (main.cu:26-33) for this lane's current path
                c.rays++;
                depthLeft--;
                float closest = __builtin_inff();
                const int k = trace<STACK>(P.S, o, d, 0.001f, closest, my, c);
                bool done = false;
                float3 contrib;
                if (k < 0) {
                    contrib = skyOf<LIT>(P, d, att);
                    done = true;
                } else {
                    HitRec h = makeHit(P.S, k, closest, o, d);
                    float3 na;
                    if (!scatter(P.S, h, d, na, g)) {
                        contrib = LIT ? emitted(h, att) : f3(0.0f, 0.0f, 0.0f);
                        if constexpr (NEE) {   // the light was sampled at the hit this ray left
                            if (fromNee && sampledLight(P.S.shade, k, h)) {
                                if constexpr (MIS)
                                    contrib = emittedWeighted(P.lights, P.lightSlot, P.nLights, h.obj, closest, d, pbs, contrib);
                                else contrib = f3(0.0f, 0.0f, 0.0f);
                            }
                        }
                        done = true;
                    } else {
                        att = mul(att, na);
                        o = h.p;
                        if (depthLeft == 0) { contrib = skyOf<LIT>(P, d, att); done = true; }
                        else if constexpr (NEE) {
                            fromNee = h.type == PT_LAMBERTIAN;
                            if (fromNee) {
                                float3 w, term;
                                if constexpr (MIS) pbs = scatterPdf(h.n, d);
                                if (lightSample<MIS>(P.lights, P.nLights, o, h.n, att, g, w, term)) {
                                    c.rays++;
                                    float tS = kShadowTmax;
                                    if (trace<STACK>(P.S, o, w, 0.001f, tS, my, c) < 0) direct = add(direct, term);
                                }
                            }
                        }
                    }
                }
                if (done) {
                    if constexpr (NEE) contrib = neeTotal(direct, contrib);
                    sum = add(sum, contrib);
                    ++sample;
                    flush();
                    if (sample == P.spp) break;
                    newPath();
                }
            }
        }
        if constexpr (!SAMPLE) {
            storePixel(P, idx, sum);
            P.sd[idx] = g.d; P.s0[idx] = g.v0; P.s1[idx] = g.v1; P.s2[idx] = g.v2; P.s3[idx] = g.v3; P.s4[idx] = g.v4;
        }
    }
    if (!SAMPLE && lane == 0) P.tileCost[tile] = (unsigned)min(__builtin_amdgcn_s_memrealtime() - tStart, 0xffffffffull);
    waveReduceAdd(P.counters + 0, c.rays);
    waveReduceAdd(P.counters + 1, c.visits);
    waveReduceAdd(P.counters + 2, c.tris);
    waveReduceAdd(P.counters + 3, c.spheres);
    waveReduceAdd(P.counters + 4, paths);
}


// Wavefront-scheduled render kernel (speculative while-while, exact).
// Each lane runs the same per-pixel program as renderKernel, decomposed into three step kinds;
// every loop iteration runs ONE kind, chosen from wave-wide __ballot counts (a uniform scalar
// branch), for all lanes that have that kind of work:
//   NODE : visit one internal node: test both child boxes against the lane's current `closest`;
//          hit leaves are appended to the lane's leaf queue (DFS order), hit internal children
//          are pushed / descended into (the reference's order: right subtree first).
//   LEAF : take the oldest queued leaf, RE-TEST its box against the current `closest`, then run
//          the primitive test (cuda_object.h:44-92).
//   SHADE: hit record + scatter + path bookkeeping + next ray (main.cu:26-36, 283-289).
// Exactness: leaves are tested in the reference's DFS order, each with the same `closest` the
// reference would use (only primitive tests change `closest`), and a box that fails with a
// stale (larger) `closest` also fails with the true one (the slab interval shrinks
// monotonically with tmax and with the box).  Node boxes tested with a stale `closest` only
// add visits.  So the sequence of primitive tests -- and every pixel -- is identical to the
// reference order; node visit counts may be higher.  Lanes keep traversing while leaves wait,
// so primitive tests run with many lanes active instead of one or two.
#ifndef PT_LEAF_QUEUE
#define PT_LEAF_QUEUE 4
#endif
constexpr int kLeafQ = PT_LEAF_QUEUE;
#ifndef PT_LEAF_QUEUE_SAMPLE
#define PT_LEAF_QUEUE_SAMPLE 2   // sample mode, binary tree, STACK <= 32; compat prefers 4 (C3 1774 vs 1959 ms)
#endif
// (PT_TASK_POOL, kTaskPool -- sample mode: tasks a wave reserves per atomic -- and PT_LDS_STACK --
// traversal stack entries per lane kept in LDS: host/pt_render_plan.hpp)
// Occupancy target of the wavefront kernel (waves per SIMD; 6 = at most 80 VGPRs).  The LDS
// stack (STACK x 256 B per wave, 160 KB per CU) allows 6 / 5 / 4 / 3 / 2 waves per SIMD at
// STACK 24 / 32 / 48 / 64 / 80, so deeper trees keep a larger register budget.  Compat tile
// mode measured best at 5 (C3 1,617 vs 1,675 ms at 6).  Sample mode on C3 (STACK 24):
// 4 waves 910 ms, 5 waves 815 ms, 6 waves 754 ms.
#ifndef PT_WAVES_PER_EU
#define PT_WAVES_PER_EU 6
#endif
template <int STACK, bool SAMPLE, bool WIDE>
constexpr int kLdsStack = (!WIDE && STACK > PT_LDS_STACK) ? PT_LDS_STACK : STACK;
#ifndef PT_WIDE_SPEC
#define PT_WIDE_SPEC 1   // wide kernels: speculative traversal, primitive groups a lane may park while it keeps visiting nodes (0-3)
#endif
#ifndef PT_WIDE_MIX
#define PT_WIDE_MIX 1   // wide kernels: plane distances by v_perm + v_fma_mix_f32 (wideHits<MIX>), bit-identical
#endif
#ifndef PT_WIDE_WAVES_PER_EU
#define PT_WIDE_WAVES_PER_EU 5   // wide tree (96 VGPRs; the stack never limits occupancy): C3 @64 spp 49.7 ms vs 68.8 at 6 (spills), 51.4 at 4
#endif
// Compat-mode wide kernels (pt_compat.hip) on shallow trees (STACK 8: C2, C3) at 4 waves per SIMD
// (104 VGPRs): C3 @1024 spp 806-825 -> 796-798 ms over three runs each, C2 @256 40.0-41.1 ->
// 41.0-41.4; deeper trees keep 5 (C5 @512: 552-558 at 5, 602-605 at 4).
#ifndef PT_COMPAT_WIDE_WAVES_PER_EU
#define PT_COMPAT_WIDE_WAVES_PER_EU 4
#endif
template <int STACK, bool SAMPLE, bool WIDE>
constexpr int kWavesPerEU = WIDE ? (SAMPLE || STACK > 8 ? PT_WIDE_WAVES_PER_EU : PT_COMPAT_WIDE_WAVES_PER_EU)
                                 : kLdsStack<STACK, SAMPLE, WIDE> <= 24
                                ? (SAMPLE ? PT_WAVES_PER_EU : 5)
                                : (kLdsStack<STACK, SAMPLE, WIDE> <= 32
                                       ? 5
                                       : (kLdsStack<STACK, SAMPLE, WIDE> <= 48 ? 4 : (STACK <= 64 ? 3 : 2)));

// WIDE: traverse the compressed 8-wide tree (wnodes / wprims, host/pt_wide8.cpp) instead of the
// binary LBVH.  Per lane: a node group `ng` (child base << 8 | hit internal slots, in slot ^ oct
// order, the nearest first), a primitive group (tgBase, tg = hit leaf primitives); NODE takes the
// next child of the group (pushing the rest), LEAF tests up to two primitives, keeping the
// minimum (t, tie rank) of wideTest -- the reference's closest hit, in any visiting order.
// Kernel arguments re-read from the kernarg segment where a rare step needs them (one scalar
// load) instead of being held in SGPRs across the step loop: the loop's uniform state exceeded
// the SGPR budget and the compiler parked the overflow in VGPR lanes, paying a v_readlane -- a
// VALU issue slot in an issue-bound kernel -- per use.  The empty asm hides the pointer's origin
// so the loads are not hoisted out of the loop again.
typedef const __attribute__((address_space(4))) RenderParams* KArgs;
__device__ __forceinline__ KArgs kargs() {
    KArgs k = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return k;
}

// The lane's bit of a wave-uniform mask as its predicate: no instruction of its own (the mask
// becomes the vcc of the v_cndmask or the exec of the branch that uses it).
__device__ __forceinline__ bool laneOf(uint64_t waveMask) { return __builtin_amdgcn_inverse_ballot_w64(waveMask); }

typedef const __attribute__((address_space(4))) float KFloat;
typedef const __attribute__((address_space(4))) uint32_t* KU32;   // read-only launch tables, scalar loads
__device__ __forceinline__ float3 ld3(const __attribute__((address_space(4))) float3& v) {
    KFloat* f = (KFloat*)&v;
    return f3(f[0], f[1], f[2]);
}
__device__ __forceinline__ DevScene ldScene(KArgs k) {
    DevScene S;
    S.nodes = k->S.nodes; S.prims = k->S.prims; S.shade = k->S.shade; S.mats = k->S.mats;
    S.wnodes = k->S.wnodes; S.wprims = k->S.wprims; S.wshade = k->S.wshade; S.wbox = k->S.wbox; S.rankOf = k->S.rankOf;
    S.iparent = k->S.iparent; S.err = k->S.err; S.nprims = k->S.nprims;
    S.hasSpheres = k->S.hasSpheres;
    S.cx = k->S.cx; S.cy = k->S.cy; S.cz = k->S.cz; S.ext = k->S.ext;
    S.mixLim = k->S.mixLim;
    S.winst = k->S.winst; S.gBits = k->S.gBits;
    return S;
}

template <bool LIT>
__device__ __forceinline__ float3 skyK(float3 d, float3 att) {
    if constexpr (LIT) return sky(d, att, ld3(kargs()->skyH), ld3(kargs()->skyZ));
    else return sky(d, att);
}

// INST (with WIDE): an instanced scene's two-level tree (pt_scene_create_instanced): a NODE step
// that reaches an instance record moves the lane's ray into the instance's object space and its
// bottom-level tree, a stack marker brings it back; no speculative traversal (a parked primitive
// group would belong to another space), no reference-order redo (instanced frames are held to a
// tolerance, not bit for bit).
// LIT: scenes with an emissive material or a sky of their own (RenderParams::lit).
// NEE (with WIDE, LIT): next-event estimation (PT_RENDER_NEE, pt.h).  A shadow ray is an
// ordinary query of the step machine whose `closest` starts at kShadowTmax: the SHADE step that
// samples a light parks the scatter direction and the pending direct term in LDS and begins the
// shadow ray from the hit point; the SHADE step that finds that query complete adds the term when
// nothing was hit and begins the parked scatter ray.  NODE and LEAF steps do not know the difference.
// MIS (with NEE): the weights of PT_RENDER_MIS (pt.h).  One more float of lane state, the scatter
// ray's pdf, beside the parked direction in LDS: written by the SHADE step that scatters, read by the
// SHADE step that finds that ray on a sampled light.
// NEE with INST (scenes built with PT_BVH_LIGHTS): the light records are world-space, one per (instance,
// emissive triangle); a SHADE step finds its lane back in the world (the marker was popped), so the
// shadow ray and the parked scatter ray start there like any bounce.
// TRI (with WIDE, not INST): the scene holds no sphere and never did (DevScene::hasSpheres == 0), known
// when the launch is enqueued (RenderParams::tri): the tests of that flag are compile-time here, and
// the sphere paths (wideTest<true>, the sphere counters, the window form of bestLo) are not compiled
// into the step loop.  TRI = false is the kernel for every scene, the flag read at run time.
// AHEAD (with SAMPLE, WIDE, TRI; not NEE): no material of the scene is metal or dielectric and the camera
// is a pinhole (RenderParams::ahead), so between its two camera draws and the end of its path a sample's
// XORWOW stream is read by the unit-sphere rejection loop alone: the k-th vector that loop accepts is the
// k-th scatter's vector whenever it is drawn.  The SHADE step runs one trial loop for the wave, only as
// long as a lane that scatters now has no vector; every other lane on a path draws along and keeps an
// accepted vector (unnormalised) in a one-entry LDS slot for its next scatter.  The metal, dielectric and
// lens code is not compiled in.
template <int STACK, bool SAMPLE, bool WIDE, bool INST = false, bool LIT = false, bool NEE = false, bool MIS = false,
          bool TRI = false, bool AHEAD = false>
// (NEE on the deeper wide stacks, 16 and 24 entries: 4 waves per SIMD instead of 5 -- at 96 VGPRs the
// SHADE step's light sample spilled 1-3 registers, and the 24-entry stack's 6 KB of LDS with the
// 2.5 KB of NEE state fit 4 waves anyway)
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(kWavesPerEU<STACK, SAMPLE, WIDE> - (NEE && STACK >= 16 ? 1 : 0)))) void renderKernelWF(RenderParams P) {
    static_assert(!NEE || (WIDE && LIT), "NEE: the wide kernels' LIT instantiations only");
    static_assert(!MIS || NEE, "MIS: the NEE instantiations only");
    static_assert(!TRI || (WIDE && !INST), "TRI: the flat wide kernels only");
    static_assert(!AHEAD || (SAMPLE && WIDE && !INST && !NEE), "AHEAD: the flat wide sample kernels without NEE only");
    // Deep trees (binary kernels) keep 32 stack entries per lane in LDS (8 KB per wave: 5 waves
    // per SIMD) and the rare deeper entries in global memory (stackSpill, per wave slot and lane).
    constexpr int LS = kLdsStack<STACK, SAMPLE, WIDE>;
    __shared__ uint32_t stk[LS * kWave];
    // Wide kernels, speculative traversal: a lane whose primitive group waits for a LEAF step
    // keeps visiting nodes; the waiting group is parked here ({base, bits} per lane; oct bit 4
    // marks it) and comes back when the current group is empty.  Not in instanced kernels.
    constexpr int SPECN = WIDE && !INST ? PT_WIDE_SPEC : 0;   // parked groups per lane: a stack, count in oct bits 4-5
    constexpr bool SPEC = SPECN > 0;
    __shared__ uint32_t pend[SPEC ? 2 * SPECN * kWave : 1];
    // instanced scenes: the lane's world ray {o, d} while it is inside an instance
    __shared__ float wray[INST ? 6 * kWave : 1];
    // sample mode: the lane's task {pixel col | local row << 16, next sample, end sample, rays}.
    // Only SHADE steps (per sample, not per node or primitive) touch it, so it lives in LDS, not
    // in four VGPRs carried through every step.
    __shared__ uint4 taskState[SAMPLE ? kWave : 1];
    // NEE: per lane, the path's direct terms so far [0..2], the pending direct term [3..5] and the
    // parked scatter direction [6..8] of a shadow query, and two flag bits -- 1: the lane's current
    // query is a shadow ray, 2: its scatter ray leaves a hit where the rule applied (a sampled light
    // it lands on contributes nothing).  Like taskState, touched by SHADE steps only: LDS, not VGPRs
    // carried through every NODE and LEAF step.  MIS: [9] the scatter ray's pdf (pbs).
    __shared__ float neeV[NEE ? (MIS ? 10 : 9) * kWave : 1];
    __shared__ uint32_t neeF[NEE ? kWave : 1];
    // AHEAD: the lane's pre-drawn scatter vector (the accepted, unnormalised centered2x3() triple);
    // haveM says whose slot is full.  Touched by SHADE steps only.
    __shared__ float aheadV[AHEAD ? 3 * kWave : 1];
    const int lane = threadIdx.x;
    // compat mode: all spp of a pixel in order (its per-pixel XORWOW stream); one wave = one tile
    // (the longest tiles split, below).
    // sample mode: persistent waves; each lane repeatedly takes a task = (pixel, summation
    // block) from a global counter and sums that block's samples in order (see PT_TAKE_TASKS).
    // `sample` runs to nSamples (compat: spp; sample mode: the end of the task's block, and
    // `sample` is the absolute sample index)
    // Compat mode, split tiles: the first splitTiles tiles of the launch order (the longest: their
    // pixels' sequential chains are the frame's critical path) run as splitWays waves each, one slice
    // of 64 / splitWays pixels per wave (the other lanes idle), so a critical pixel shares its wave's
    // steps with fewer other pixels and its chain advances in more of them.
    int bidT = (int)blockIdx.x, slice = -1;
    // compat, critical-pixel waves (CRIT): the first critWaves blocks (wave-uniform)
    constexpr bool CRITK = critFor(SAMPLE, WIDE, INST, STACK);
    const bool crit = CRITK && bidT < P.critWaves;
    if constexpr (CRITK) {
        if (!crit) bidT -= P.critWaves;
    }
    if constexpr (!SAMPLE) {
        const int ks = P.splitTiles * P.splitWays;   // (uniform)
        if (crit) {
        } else if (bidT < ks) { slice = bidT % P.splitWays; bidT /= P.splitWays; }
        else bidT -= ks - P.splitTiles;
    }
    int tile = (SAMPLE || crit) ? -1 : tileOf(P, bidT), nSamples = SAMPLE ? 0 : P.spp;
    int col = 0, lrow = 0;
    bool valid = false;
    uint32_t idx = 0u;
    if constexpr (!SAMPLE) {
        if (crit) {   // a listed pixel per lane (lanes beyond critLanes or the list idle)
            const int k = bidT * P.critLanes + lane;
            valid = lane < P.critLanes && k < P.nCrit;
            idx = valid ? P.critList[k] : 0u;
            col = (int)(idx % (uint32_t)P.width);
            lrow = (int)(idx / (uint32_t)P.width);
        } else {
            col = (tile % P.tiles_x) * 8 + (lane & 7);
            lrow = (tile / P.tiles_x) * 8 + (lane >> 3);
            valid = col < P.width && lrow < P.nrows && (slice < 0 || (lane * P.splitWays) / kWave == slice);
            idx = valid ? (uint32_t)lrow * (uint32_t)P.width + (uint32_t)col : 0u;   // npix < 2^32
            if (CRITK && valid && P.critFlag && P.critFlag[idx]) valid = false;   // (a critical wave's pixel)
        }
    }
    const unsigned long long tStart = __builtin_amdgcn_s_memrealtime();
    if (!SAMPLE && !crit && bidT < P.prioTiles) {   // wave-uniform condition (s_setprio takes an immediate)
        if (P.prioLevel >= 3) __builtin_amdgcn_s_setprio(3);
        else if (P.prioLevel == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
    }
    float fcol = (float)col;
    float frow = valid ? (float)globalRow(lrow, P.stripe_h, P.nparts, P.part) : 0.0f;
    const DevScene& S = P.S;
    // gfx9 buffer resource: base = the node array, raw (stride 0), DATA_FORMAT_32 in dword 3
    const __amdgpu_buffer_rsrc_t nodeRsrc = rawRsrc(WIDE ? (const void*)S.wnodes : (const void*)S.nodes);
    uint32_t* my = stk + lane;
    // Work counters are wave totals kept in scalar registers: each step adds the popcount of
    // a ballot of the lanes that did the work (no per-lane counter VGPRs; waveCount).
    // The compat unit's kernels (CTU: pt_compat.hip) keep the plain sum.  Those with critical-pixel
    // waves must: PT_CRIT_TRACE counts inside a per-lane loop that lanes leave at different
    // iterations, so their counters are per-lane values (lane 0's is reported).  The stack-16 and -24
    // ones may not: one of them takes two more VGPRs with scalar counters, and CTU also keeps rcpRN
    // per component at the ray start, where the one-check form costs the triangle-only stack-8
    // kernel its fifth wave (97 VGPRs).
    constexpr bool CTU = !SAMPLE && WIDE && !INST;
#define PT_COUNT(v, x)                                                                              \
    do {                                                                                          \
        if constexpr (CTU) (v) += (x);                                                            \
        else waveCount((v), (x));                                                                 \
    } while (0)
    uint32_t sRays = 0, sVisits = 0, sTris = 0, sSph = 0, sPaths = 0;
#ifdef PT_DIAG
    uint32_t itN = 0, itL = 0, itS = 0, sPops = 0, sRedo = 0;   // scheduler diagnostics (iterations per kind)
    uint32_t sRedoMiss = 0;   // redone queries whose final hit's exact box the ray misses outright (deferredRedo)
    unsigned long long sSpecN = 0, sIdleN = 0;   // NODE steps: lanes waiting on primitives that have nodes left; lanes with no NODE work
    unsigned long long sHalf = 0, sParkT = 0;    // LEAF (wide): lanes testing one primitive; tests in parked groups
    unsigned long long cycN = 0, cycL = 0, cycS = 0, cycH = 0;   // and shader cycles per kind, loop head
    unsigned long long cycSh = 0, cycTk = 0, cycNp = 0, cycBr = 0;   // SHADE: shading, tasks, new path, ray start
    unsigned long long sTrials = 0;   // SHADE: iterations of the unit-sphere trial loop (the wave's, per step)
#define PT_DIAG_ADD(v, x) (v) += (x)
#else
#define PT_DIAG_ADD(v, x) ((void)0)
#endif

    Xorwow g{};
    if constexpr (!SAMPLE) {
        if (valid) g = Xorwow{P.sd[idx], P.s0[idx], P.s1[idx], P.s2[idx], P.s3[idx], P.s4[idx]};
    }
    float3 sum = f3(0.0f, 0.0f, 0.0f), o = f3(0.0f, 0.0f, 0.0f), d = f3(0.0f, 0.0f, 1.0f);
    float3 inv = d, att = f3(1.0f, 1.0f, 1.0f);
    float closest = 0.0f;
    int best = -1, depthLeft = 0, sample = 0, node = -1, sp = 0, qn = 0;
    // leaf queue depth: sample mode on shallow trees (STACK <= 32: C2, C3) prefers 2, deep trees
    // (C5, STACK 48+) and compat mode 4 (C3 1068 vs 1088 ms, C2 67.4 vs 70.6, C5 1576 vs 1471)
    constexpr int LQ = (SAMPLE && !WIDE && STACK <= 32) ? PT_LEAF_QUEUE_SAMPLE : kLeafQ;
    uint32_t qref[LQ];   // leaf queue: leaf refs in DFS order (registers: constant indices only)
    float lq[LQ];     // their slab entry distances
#pragma unroll
    for (int i = 0; i < LQ; i++) { qref[i] = 0u; lq[i] = 0.0f; }
    // wide tree traversal state (WIDE): node group, primitive group, ray octant (| 8: redo the
    // query in the reference's order), the best hit's window end (scenes with spheres, instanced
    // scenes) or the second-smallest candidate distance t2 (triangle-only scenes: wideTestTri)
    uint32_t ng = 0u, tgBase = 0u, tg = 0u, oct = 0u;
    float bestLo = 0.0f;
    // Scheduler predicates are wave masks (one bit per lane, an SGPR pair each), combined with
    // scalar logic and turned back into a lane predicate by laneOf() where a step needs one: a
    // __ballot of a bool that went through && / || or a join costs two VALU (v_cndmask 0, 1 and
    // v_cmp_ne) to rebuild a mask that already exists, so only plain integer compares are balloted.
    const uint64_t allM = __ballot(true);
    uint64_t activeM = 0;   // lanes on a path
    uint64_t haveM = 0;     // AHEAD: lanes whose slot holds their path's next scatter vector
    // sample mode task state: summation block, its tile (cost accounting), rays traced for it
    uint32_t depthPaths = 0;
    uint32_t pxRays = 0;   // compat tile / critical lanes: rays traced for the lane's pixel (P.pixRays)
    uint64_t needTaskM = SAMPLE ? allM : 0;   // sample mode: lanes waiting for a task
    uint32_t poolBase = 0u, poolLeft = 0u;   // sample mode: the wave's reserved tasks (uniform)


    // Start the closest-hit query of (o, d).  (Macros, not lambdas: a [&] closure makes the
    // captured variables address-taken and they end up in scratch memory.)
    // SH (NEE kernels; a constant false elsewhere): the query is a shadow ray -- it starts at
    // kShadowTmax instead of +inf, uses up no bounce and is never the camera's ray.
#define PT_BEGIN_RAY(SH)                                                                            \
    do {                                                                                          \
        const bool sh_ = NEE && (SH);                                                             \
        if constexpr (NEE) depthLeft -= sh_ ? 0 : 1;                                              \
        else depthLeft--;                                                                         \
        if constexpr (SAMPLE) {   /* rays per task: only frames that measure tile costs use them */ \
            if (kargs()->measureCost)                                                             \
                __hip_atomic_fetch_add(&taskState[lane].w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
        }                                                                                         \
        closest = sh_ ? kShadowTmax : __builtin_inff();                                           \
        best = -1;                                                                                \
        sp = 0;                                                                                   \
        qn = 0;                                                                                   \
        if constexpr (CRITK) pxRays++;                                                            \
        if constexpr (WIDE) {   /* the root is slot 0 of a virtual node at base 0 */              \
            if constexpr (CTU) inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));                      \
            else inv = rcpRN3Wave(d);                                                             \
            const uint32_t oc_ = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u); \
            oct = oc_;                                                                            \
            tg = 0u;                                                                              \
            /* sphere scenes: the best hit's window end; triangle-only: t2 (wideTestTri) */        \
            /* (t2 counts the start value of a finite interval as a candidate: deferredRedo then  \
               sends a final hit whose box entry lies beyond it to the reference-order query,    \
               which is what wideTest's `closest < b.lo` does for the ray-query kernels) */       \
            if constexpr (TRI) bestLo = closest;                                                  \
            else bestLo = INST || kargs()->S.hasSpheres ? -__builtin_inff() : closest;            \
            ng = S.nprims > 0 ? (1u << oc_) : 0u;                                                 \
            /* only camera rays can start far from the scene (a bounce starts on a primitive), and  \
               they all start at the camera: one uniform flag, set on the host (wideFar) */     \
            if (!INST && ((kargs()->camFar && !sh_ && depthLeft + 1 == kargs()->max_depth) ||      \
                          (PT_WIDE_MIX && mixUnsafe(inv, kargs()->S.mixLim)))) {                   \
                ng = 0u;       /* origin far from the scene, or a direction the MIX planes */      \
                oct |= 8u;     /* cannot take: the query in the reference's order (SHADE's redo) */ \
            }                                                                                     \
            if (INST && kargs()->camFar && !sh_ && depthLeft + 1 == kargs()->max_depth) {          \
                /* a far camera: the path starts where its ray enters the world (instEntry) */     \
                const auto& K_ = *kargs();                                                        \
                (void)instEntry(K_.S.cx, K_.S.cy, K_.S.cz, K_.S.ext, o, d, inv);                   \
            }                                                                                     \
            if (CRITK && crit) PT_CRIT_TRACE();                                                    \
        } else if (S.nprims <= 1) {                                                               \
            node = -1;                                                                            \
            if (S.nprims == 1) { /* root is a leaf: no box test (render_manager.h:92-98) */       \
                const float t1 = primHitT(loadPrim(S, 0), __float_as_uint(S.prims[2].w) != 0, o, d, \
                                          0.001f, closest);                                       \
                if (t1 >= 0.0f) { closest = t1; best = 0; }                                       \
            }                                                                                     \
        } else {                                                                                  \
            inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));                                         \
            node = 0;                                                                             \
        }                                                                                         \
    } while (0)
    // Critical-pixel waves (compat, wide): the lane's whole closest-hit query at once, in a per-lane
    // loop (nearest child first, the NODE and LEAF steps' own tests and tie / window rules, no
    // speculation): a lane alone on its chain advances every iteration instead of waiting for the
    // wave's step kinds.  The result is the reference's closest hit either way;
    // a flagged order-dependent query is redone in the reference's order by the SHADE step as usual.
#define PT_CRIT_TRACE()                                                                             \
    do {                                                                                          \
        const bool lb_ = S.nprims > 1;                                                            \
        bool sph_ = false;                                                                        \
        if constexpr (!TRI) sph_ = kargs()->S.hasSpheres != 0;                                    \
        bool redo_ = false;                                                                       \
        for (;;) {                                                                                \
            while (tg) {                                                                          \
                const uint32_t k_ = tgBase + (uint32_t)__builtin_ctz(tg);                         \
                tg &= tg - 1u;                                                                    \
                const float4* w_ = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.wprims) + mul48(k_)); \
                const Prim q_{w_[0], w_[1], w_[2]};                                               \
                if constexpr (TRI) {   /* (no record is a sphere) */                              \
                    PT_COUNT(sTris, (uint32_t)__popcll(__ballot(true)));                          \
                    wideTestTri(q_, __ballot(true), o, d, 0.001f, closest, best, bestLo);         \
                } else {                                                                          \
                const bool isS_ = __float_as_uint(q_.p2.w) != 0u;                                 \
                PT_COUNT(sTris, (uint32_t)__popcll(__ballot(!isS_)));                             \
                PT_COUNT(sSph, (uint32_t)__popcll(__ballot(isS_)));                               \
                if (sph_) wideTest<true>(q_, o, d, inv, 0.001f, closest, best, bestLo, lb_, redo_, 0u); \
                else if (INST) wideTest<false>(q_, o, d, inv, 0.001f, closest, best, bestLo, lb_, redo_, 0u); \
                else wideTestTri(q_, __ballot(true), o, d, 0.001f, closest, best, bestLo);   /* (SHADE decides) */ \
                }                                                                                 \
            }                                                                                     \
            if ((ng & 0xffu) == 0u) {                                                             \
                if (sp == 0) break;                                                               \
                sp--;                                                                             \
                ng = my[sp * kWave];                                                              \
            }                                                                                     \
            const uint32_t bit_ = (uint32_t)__builtin_ctz(ng & 0xffu);                            \
            const uint32_t child_ = (ng >> 8) + (bit_ ^ (oct & 7u));                              \
            ng &= ~(1u << bit_);                                                                  \
            if (ng & 0xffu) { my[sp * kWave] = ng; sp++; }   /* sp < depth <= STACK (host check) */ \
            PT_COUNT(sVisits, (uint32_t)__popcll(__ballot(true)));                                \
            const uint32_t off_ = mul80(child_);                                                  \
            const uint4 n0_ = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off_, 0, 0)); \
            const uint4 n1_ = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off_ + 16u, 0, 0)); \
            const uint4 n2_ = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off_ + 32u, 0, 0)); \
            const uint4 n3_ = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off_ + 48u, 0, 0)); \
            const uint4 n4_ = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off_ + 64u, 0, 0)); \
            const uint32_t h_ = wideHits<PT_WIDE_MIX != 0>(n0_, n1_, n2_, n3_, n4_, o, inv, oct & 7u, 0.001f, closest); \
            ng = (n1_.x << 8) | (h_ >> 24);                                                      \
            tgBase = n1_.y;                                                                       \
            tg = h_ & 0xffffffu;                                                                  \
        }                                                                                         \
        if (redo_) oct |= 8u;   /* order-dependent candidate: SHADE repeats the query */           \
    } while (0)
    // Sample mode: the lanes of needTaskM take the next tasks of the wave's pool, in lane order; an
    // empty pool is refilled with the next kTaskPool tasks of the global counter (one returning
    // atomic, whose latency the wave waits out, per kTaskPool tasks instead of per SHADE step).
    // Task t = (tile slot t / 64 / nblocks in launch order, block (t / 64) % nblocks, pixel
    // t % 64 of the 8x8 tile); tasks off the frame edge are skipped.  Sets the bits of `got` for
    // lanes that received a task; lanes that find the counter exhausted stop asking.  Every lane
    // decodes a task (the same instructions whatever the exec mask); who took one, ran out or fell
    // off the frame is wave masks.
#define PT_TAKE_TASKS(got)                                                                          \
    do {                                                                                          \
        const auto& Q_ = *kargs();                                                                \
        for (;;) {                                                                                \
            const uint64_t m_ = needTaskM;                                                        \
            if (m_ == 0) break;                                                                   \
            if (poolLeft == 0u) { /* refill the wave's pool: one returning atomic per kTaskPool */ \
                const int leader_ = __ffsll((unsigned long long)m_) - 1;                          \
                /* always a full pool: = one (tile, block) group, one task per lane; smaller    \
                   grabs near the end measured slower (1/8 share: 150-158 vs 145 ms) */          \
                const uint32_t grab_ = (uint32_t)kTaskPool;                                       \
                uint32_t b_ = 0;                                                                  \
                if (lane == leader_) b_ = atomicAdd(Q_.taskCounter, grab_);                       \
                poolBase = __builtin_amdgcn_readfirstlane((uint32_t)__shfl((int)b_, leader_));    \
                poolLeft = grab_;                                                                 \
            }                                                                                     \
            /* wave-uniform: the taken tasks span task groups (tile slot, block) g0 and g0 + 1 */  \
            const uint32_t base_ = poolBase;                                                      \
            const uint32_t take_ = min((uint32_t)__popcll(m_), poolLeft);                         \
            poolBase += take_;                                                                    \
            poolLeft -= take_;                                                                    \
            const uint32_t g0_ = base_ >> 6, off_ = base_ & 63u;                                  \
            const uint32_t slotA_ = Q_.nblocksShift >= 0 ? g0_ >> Q_.nblocksShift : g0_ / (uint32_t)Q_.ngroups; \
            const uint32_t blkA_ = g0_ - slotA_ * (uint32_t)Q_.ngroups;                           \
            const bool wrap_ = blkA_ + 1u == (uint32_t)Q_.ngroups;                                  \
            const uint32_t slotB_ = wrap_ ? slotA_ + 1u : slotA_, blkB_ = wrap_ ? 0u : blkA_ + 1u; \
            const uint32_t nslots_ = (uint32_t)Q_.ntiles;                                          \
            /* the slots' tiles, decoded once per launch order (tileXYKernel): no divisions here */ \
            /* (scalar loads through the constant address space: a vector load here would wait   \
               out the accumulator atomics a finishing lane has just issued -- vmcnt counts every \
               vector memory operation in issue order) */                                        \
            const uint32_t xyA_ = slotA_ < nslots_ ? ((KU32)Q_.tileXY)[__builtin_amdgcn_readfirstlane(slotA_)] : 0u; \
            const uint32_t xyB_ = slotB_ < nslots_ ? ((KU32)Q_.tileXY)[__builtin_amdgcn_readfirstlane(slotB_)] : 0u; \
            const uint32_t txA_ = xyA_ & 0xffffu, tyA_ = xyA_ >> 16;                              \
            const uint32_t txB_ = xyB_ & 0xffffu, tyB_ = xyB_ >> 16;                              \
            const uint32_t k_ = (uint32_t)__popcll(m_ & ((1ull << lane) - 1ull));                 \
            const uint32_t o_ = off_ + k_, px_ = o_ & 63u;                                        \
            const bool hi_ = o_ >= 64u;                                                           \
            const int c_ = (int)((hi_ ? txB_ : txA_) * 8u + (px_ & 7u));                          \
            const int r_ = (int)((hi_ ? tyB_ : tyA_) * 8u + (px_ >> 3));                          \
            const uint64_t took_ = m_ & __ballot(k_ < take_);                                     \
            const uint64_t left_ = took_ & __ballot(base_ + k_ < Q_.ntasks);                      \
            const uint64_t in_ = left_ & __ballot(c_ < Q_.width) & __ballot(r_ < Q_.nrows);       \
            needTaskM &= ~((took_ & ~left_) | in_);                                               \
            got |= in_;                                                                           \
            if (laneOf(in_)) {                                                                    \
                /* (both groups' first samples are wave-uniform: scalar products, one select) */  \
                const uint32_t sA_ = blkA_ * (uint32_t)Q_.span, sB_ = blkB_ * (uint32_t)Q_.span;  \
                const uint32_t s0_ = hi_ ? sB_ : sA_;                                             \
                taskState[lane] = make_uint4((uint32_t)c_ | ((uint32_t)r_ << 16), s0_,             \
                                             min(s0_ + (uint32_t)Q_.span, (uint32_t)Q_.spp), 0u); \
                sum = f3(0.0f, 0.0f, 0.0f);                                                       \
            }                                                                                     \
        }                                                                                         \
    } while (0)
    // Sample mode: the lane's block (= its task; ts = the task state) is complete: its sum and ray
    // count go to the pixel's accumulator (order-free integer atomics on per-pixel addresses: no
    // contention; right here -- deferring them to a later step of the loop, where fewer registers
    // are live, measured 2.6 % slower); the caller moves the lane's bit to needTaskM.
#define PT_FINISH_TASK(ts)                                                                          \
    do {                                                                                          \
        /* (a 24-bit multiply-add: sample mode's local rows and width are < 2^16, launchRender) */ \
        unsigned long long* acc_ = kargs()->pixAcc + 4 * (size_t)(__umul24((ts).x >> 16, (uint32_t)kargs()->width) + ((ts).x & 0xffffu)); \
        addBlock(acc_, sum, (ts).w + 1u, kargs()->measureCost != 0);                              \
    } while (0)
    // New camera sample: main.cu:284-286 + camera::get_ray (lens sample: lensOffset; time draw skipped).
#define PT_NEW_PATH()                                                                               \
    do {                                                                                          \
        const auto& Q_ = *kargs();                                                                \
        if constexpr (SAMPLE) {   /* the task's pixel and next sample from LDS */                \
            const uint4 ts_ = taskState[lane];                                                    \
            fcol = (float)(ts_.x & 0xffffu);                                                      \
            const uint32_t grow_ = (uint32_t)globalRowFast((int)(ts_.x >> 16), Q_.stripe_h, Q_.stripeShift, \
                                                           Q_.nparts, Q_.part);                  \
            frow = (float)grow_;                                                                  \
            g = sampleStream<true>(Q_.seed0, Q_.seed1, Q_.sampleBase + ts_.y,                     \
                             grow_ * (uint32_t)Q_.width + (ts_.x & 0xffffu));                      \
        }                                                                                         \
        const float u_ = (fcol + g.uniform()) * Q_.invW;                                           \
        const float v_ = (frow + g.uniform()) * Q_.invH;                                           \
        o = ld3(Q_.cam.pos);                                                                            \
        d = sub(add(add(ld3(Q_.cam.ll), scale(u_, ld3(Q_.cam.hor))), scale(v_, ld3(Q_.cam.ver))), ld3(Q_.cam.pos));       \
        if (!AHEAD && Q_.cam.lens != 0.0f) lensOffset(ld3(Q_.cam.right), ld3(Q_.cam.up), Q_.cam.lens, g, o, d); \
        att = f3(1.0f, 1.0f, 1.0f);                                                               \
        depthLeft = Q_.max_depth;                                                                  \
        if constexpr (NEE) {   /* no direct term yet, no flag */                                  \
            neeV[0 * kWave + lane] = 0.0f; neeV[1 * kWave + lane] = 0.0f; neeV[2 * kWave + lane] = 0.0f; \
            neeF[lane] = 0u;                                                                      \
        }                                                                                         \
    } while (0)

    // The sky colour of (d, att); LIT: the scene's horizon and zenith from the kernel arguments (six
    // scalar loads where a path ends, not six registers held across the step loop).
#define PT_SKY() skyK<LIT>(d, att)

    bool started = false;
    if constexpr (SAMPLE) {
        // Every lane starts in needTaskM: the first loop iteration is a SHADE step that hands
        // out tasks.  max_depth <= 0 (no bounce: each sample is the sky colour of its camera
        // ray) is handled here, without the loop.
        if (P.max_depth <= 0) {
            for (;;) {
                uint64_t got = 0;
                PT_TAKE_TASKS(got);
                if (got == 0) break;
                needTaskM |= got;   // (each of them ends its task below)
                if (laneOf(got)) {
                    uint4 ts = taskState[lane];
                    depthPaths += ts.z - ts.y;
                    while (ts.y < ts.z) {
                        taskState[lane].y = ts.y;
                        PT_NEW_PATH();
                        sum = add(sum, endOf<NEE>(f3(0.0f, 0.0f, 0.0f), PT_SKY()));
                        ts.y++;
                        // (a kernarg pointer re-read with no user -- kargs' empty asm is volatile --
                        // that the register assignment of the sample kernels was measured with)
                        if (ts.y < ts.z) (void)kargs();
                    }
                    PT_FINISH_TASK(ts);
                }
            }
            needTaskM = 0;
            waveReduceAdd(P.counters + 4, depthPaths);   // (paths counted per lane here)
        }
    } else if (valid) {
        if (P.max_depth <= 0) {
            for (; sample < nSamples; sample++) {
                PT_NEW_PATH();
                sum = add(sum, endOf<NEE>(f3(0.0f, 0.0f, 0.0f), PT_SKY()));
            }
        } else if (nSamples > 0) {
            PT_NEW_PATH();
            PT_BEGIN_RAY(false);
            started = true;
        }
    }
    activeM = __ballot(started);   // (once per wave)
    PT_COUNT(sRays, (uint32_t)__popcll(activeM));
    PT_COUNT(sPaths, (uint32_t)__popcll(activeM) +
                                 (!SAMPLE && P.max_depth <= 0 ? (uint32_t)__popcll(__ballot(valid)) * (uint32_t)nSamples : 0u));

    for (;;) {
#ifdef PT_DIAG
        const unsigned long long tH0 = __builtin_amdgcn_s_memtime();
#endif
        // binary: room for both children's leaves in the queue; wide: nodes left, and no primitives
        // pending or (speculative traversal) room to park them.  Instanced kernels never park
        // (SPEC is false there).  One ballot per integer compare, the rest is scalar logic.
        uint64_t mN, mL, mS;
        if constexpr (WIDE) {
            const uint64_t noPrims = __ballot(tg == 0u);
            const uint64_t nodesLeft = __ballot(((ng & 0xffu) | (uint32_t)sp) != 0u);   // (sp >= 0)
            uint64_t mayVisit = noPrims;
            if constexpr (SPEC)
                mayVisit |= __ballot(SPECN == 1 ? (oct & 48u) == 0u : ((oct >> 4) & 3u) < (uint32_t)SPECN);
            mN = mayVisit & nodesLeft;
            mL = allM & ~noPrims;
            mS = (activeM & noPrims & ~nodesLeft) | needTaskM;
        } else {
            const uint64_t inTree = __ballot(node >= 0), queued = __ballot(qn > 0);   // (node >= -1)
            mN = inTree & (LQ == 2 ? allM & ~queued : __ballot(qn <= LQ - 2));
            mL = queued;
            mS = (activeM & ~inTree & ~queued) | needTaskM;
        }
        if ((mN | mL | mS) == 0) break;
        const int nN = __popcll(mN), nL = __popcll(mL), nS = __popcll(mS);
        int kind;   // 0 node, 1 leaf, 2 shade
        if (nN == 0) kind = nL > 0 ? 1 : 2;
        else if (nL >= P.leafBatch) kind = 1;
        else if (nS >= P.shadeBatch) kind = 2;
        else if (!SAMPLE && nN < P.nodeMin && (nL | nS)) kind = nL >= nS ? 1 : 2;
        else kind = 0;
#ifdef PT_DIAG
        const unsigned long long tK0 = __builtin_amdgcn_s_memtime();
        cycH += tK0 - tH0;
#endif

        if (kind == 0) {
            // ------------------------------------------------------------------ NODE
            PT_COUNT(sVisits, (uint32_t)nN);
            PT_DIAG_ADD(itN, 1u);
            const bool wantNode = laneOf(mN);
            if constexpr (WIDE) {
                PT_DIAG_ADD(sSpecN, (unsigned long long)__popcll(__ballot(tg != 0u && ((ng & 0xffu) != 0u || sp > 0))));
                PT_DIAG_ADD(sIdleN, (unsigned long long)(64 - nN));
            }
            if constexpr (INST) {
                if (wantNode) {
                    // pop to a group with children left; a marker returns the lane to the world
                    // (oct bit 3: the instance transformed the direction, not only the origin)
                    while ((ng & 0xffu) == 0u && sp > 0) {
                        sp--;
                        ng = my[sp * kWave];
                        if (ng == kInstMarker) {
                            o = f3(wray[0 * kWave + lane], wray[1 * kWave + lane], wray[2 * kWave + lane]);
                            if (oct & 8u) {
                                d = f3(wray[3 * kWave + lane], wray[4 * kWave + lane], wray[5 * kWave + lane]);
                                inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));
                                oct = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
                            } else {
                                oct &= 7u;
                            }
                            ng = 0u;
                        }
                    }
                    if (ng & 0xffu) {
                        const uint32_t bit = (uint32_t)__builtin_ctz(ng & 0xffu);
                        const uint32_t child = (ng >> 8) + (bit ^ (oct & 7u));
                        ng &= ~(1u << bit);
                        if (ng & 0xffu) { my[sp * kWave] = ng; sp++; }
                        uint32_t off = mul80(child);
                        uint4 n0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off, 0, 0));
                        uint4 n1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 16u, 0, 0));
                        uint4 n2 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 32u, 0, 0));
                        uint4 n3 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 48u, 0, 0));
                        uint4 n4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 64u, 0, 0));
                        if (n0.w == kInstFlag) {   // an instance: into its object space, and its tree's root in this step
                            wray[0 * kWave + lane] = o.x; wray[1 * kWave + lane] = o.y; wray[2 * kWave + lane] = o.z;
                            uint32_t full = 0u;
                            if (n0.x == 0u) {   // (an identity instance keeps the world ray)
                                const float4 r0 = __builtin_bit_cast(float4, n2), r1 = __builtin_bit_cast(float4, n3),
                                             r2 = __builtin_bit_cast(float4, n4);
                                if (n0.y != 0u) {   // translation only: the same origin as xformPoint, the direction kept
                                    o = f3(o.x + r0.w, o.y + r1.w, o.z + r2.w);
                                } else {
                                    wray[3 * kWave + lane] = d.x; wray[4 * kWave + lane] = d.y; wray[5 * kWave + lane] = d.z;
                                    o = xformPoint(r0, r1, r2, o);
                                    d = xformDir(r0, r1, r2, d);
                                    inv = f3(rcpRN(d.x), rcpRN(d.y), rcpRN(d.z));
                                    full = 8u;
                                }
                            }
                            const uint32_t oc = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
                            my[sp * kWave] = kInstMarker;   // (depth: host check, wideStackFor)
                            sp++;
                            oct = oc | full | (n1.y << 8);   // bits 8+: the instance the lane is in
                            off = mul80(n1.x);               // the mesh tree's root
                            n0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off, 0, 0));
                            n1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 16u, 0, 0));
                            n2 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 32u, 0, 0));
                            n3 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 48u, 0, 0));
                            n4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 64u, 0, 0));
                        }
                        const uint32_t hits = wideHitsInst(n0, n1, n2, n3, n4, o, inv, oct & 7u, 0.001f, closest);
                        ng = (n1.x << 8) | (hits >> 24);
                        tgBase = n1.y;
                        tg = hits & 0xffffffu;
                    }
                }
            } else if constexpr (WIDE) {
                if (wantNode) {
                    if (SPEC && laneOf(mL)) {   // park the waiting primitive group (tg != 0), keep traversing
                        const uint32_t c = SPECN == 1 ? 0u : (oct >> 4) & 3u;
                        pend[(2u * c) * kWave + lane] = tgBase;
                        pend[(2u * c + 1u) * kWave + lane] = tg;
                        oct += 16u;
                    }
                    // (the parked values are read back from LDS, not kept in registers meanwhile)
                    if constexpr (SPEC) asm volatile("" ::: "memory");
                    if ((ng & 0xffu) == 0u) { sp--; ng = my[sp * kWave]; }   // the group below
                    const uint32_t bit = (uint32_t)__builtin_ctz(ng & 0xffu);   // nearest remaining child
                    const uint32_t child = (ng >> 8) + (bit ^ (oct & 7u));
                    ng &= ~(1u << bit);
                    if (ng & 0xffu) { my[sp * kWave] = ng; sp++; }   // sp < depth <= STACK (host check)
                    const uint32_t off = mul80(child);
                    const uint4 n0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off, 0, 0));
                    const uint4 n1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 16u, 0, 0));
                    const uint4 n2 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 32u, 0, 0));
                    const uint4 n3 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 48u, 0, 0));
                    const uint4 n4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 64u, 0, 0));
                    const uint32_t hits = wideHits<PT_WIDE_MIX != 0, TRI && SAMPLE>(n0, n1, n2, n3, n4, o, inv, oct & 7u, 0.001f, closest);
                    ng = (n1.x << 8) | (hits >> 24);
                    tgBase = n1.y;
                    tg = hits & 0xffffffu;
#ifdef PT_DIAG
                    oct &= ~64u;   // (diagnostics: bit 6 marks a group that was parked)
#endif
                    if (SPEC && tg == 0u && (oct & 48u)) {   // no new primitives: the last parked group is current again
                        oct -= 16u;
                        const uint32_t c = SPECN == 1 ? 0u : (oct >> 4) & 3u;
                        tgBase = pend[(2u * c) * kWave + lane];
                        tg = pend[(2u * c + 1u) * kWave + lane];
#ifdef PT_DIAG
                        oct |= 64u;
#endif
                    }
                }
            } else if (wantNode) {
                // buffer loads: a 32-bit per-lane offset off a wave-uniform resource (no 64-bit
                // address arithmetic per visit); < 2^26 nodes (pt_scene_create)
                const uint32_t off = (uint32_t)node * 64u;
                const float4 a = bload4(nodeRsrc, off), b = bload4(nodeRsrc, off + 16u);
                const float4 q = bload4(nodeRsrc, off + 32u), r = bload4(nodeRsrc, off + 48u);
                const uint32_t lref = __float_as_uint(r.x), rref = __float_as_uint(r.y);
                SlabHit2 h2 = slabBoth(a, b, q, o, inv, 0.001f, closest);
                // keep the right child's packed arithmetic next to the left's (not sunk past the
                // left child's queue append, where the operand pairs are no longer at hand)
                asm volatile("" : "+v"(h2.r.lo));
                const SlabHit hl = h2.l, hr = h2.r;
                // append hit leaves in order (left, then right) with their slab entry distances
                if constexpr (LQ == 2) {
                    // a NODE step needs an empty queue (qn <= LQ - 2): the slots are fixed
                    const bool al = hl.hit && (lref & kLeafBit), ar = hr.hit && (rref & kLeafBit);
                    qref[0] = al ? lref : rref;
                    lq[0] = al ? hl.lo : hr.lo;
                    qref[1] = rref;
                    lq[1] = hr.lo;
                    qn = (al ? 1 : 0) + (ar ? 1 : 0);
                } else {
                if (hl.hit && (lref & kLeafBit)) {
#pragma unroll
                    for (int i = 0; i < LQ; i++) {
                        qref[i] = qn == i ? lref : qref[i];
                        lq[i] = qn == i ? hl.lo : lq[i];
                    }
                    qn++;
                }
                if (hr.hit && (rref & kLeafBit)) {
#pragma unroll
                    for (int i = 0; i < LQ; i++) {
                        qref[i] = qn == i ? rref : qref[i];
                        lq[i] = qn == i ? hr.lo : lq[i];
                    }
                    qn++;
                }
                }
                const bool il = hl.hit && !(lref & kLeafBit), ir = hr.hit && !(rref & kLeafBit);
                // push left then right, pop: descend straight into the child that would be popped.
                // No overflow check: an entry is pushed only for a left sibling on the current
                // path, one per level, so sp < depth <= STACK - 1 (stackFor).
                if (ir) {
                    if (il) {
                        if (LS == STACK || sp < LS) my[sp * kWave] = lref;
                        else P.stackSpill[((size_t)blockIdx.x * kWave + lane) * (STACK - LS) + (sp - LS)] = lref;
                        sp++;
                    }
                    node = (int)rref;
                } else if (il) {
                    node = (int)lref;
                } else if (sp > 0) {
                    sp--;
                    node = (LS == STACK || sp < LS)
                               ? (int)my[sp * kWave]
                               : (int)P.stackSpill[((size_t)blockIdx.x * kWave + lane) * (STACK - LS) + (sp - LS)];
                } else {
                    node = -1;
                }
            }
        }
        if (kind == 1) {
            // ------------------------------------------------------------------ LEAF
            bool tested = false, sph = false;
            PT_DIAG_ADD(itL, 1u);
            if constexpr (WIDE) {
                PT_DIAG_ADD(sPops, (uint32_t)nL);
                // up to two primitives of the group per step, both records loaded up front
                uint32_t k0 = 0u, k1 = 0u;
                const bool h0 = laneOf(mL);
                if (h0) k0 = tgBase + (uint32_t)__builtin_ctz(tg);
                tg &= tg - 1u;   // (every lane: an empty group stays empty)
                // (tg < 2^24.  The signed compare keeps the ballot a compare of its own: `tg != 0u`
                // is merged with the `tg - 1u` below into one subtract whose carry-out is the
                // predicate, and a ballot of that carry rebuilds the mask through a VGPR)
                const uint64_t m1 = __ballot((int)tg > 0);
                const bool h1 = laneOf(m1);
                if (h1) k1 = tgBase + (uint32_t)__builtin_ctz(tg);
                tg &= tg - 1u;
                // Every lane loads two records (lanes without a primitive read record 0): a
                // conditional load would cost a zero fill of 24 registers per step
                // 32-bit byte offsets off the uniform base (global loads with an SGPR base): no
                // 64-bit address arithmetic, no quarter-rate multiply
                const float4* w0 = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.wprims) + mul48(k0));
                const float4* w1 = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.wprims) + mul48(k1));
                const Prim q0{w0[0], w0[1], w0[2]}, q1{w1[0], w1[1], w1[2]};
                bool redo = false;
#ifdef PT_DIAG
                {
                    sHalf += (unsigned long long)__popcll(__ballot(h0 && !h1));
                    const bool pk = !INST && (oct & 64u) != 0u;
                    sParkT += (unsigned long long)(__popcll(__ballot(pk && h0)) + __popcll(__ballot(pk && h1)));
                }
#endif
                // (instanced: no reference leaf-box rule; the hit key carries the instance)
                const bool lb = !INST && S.nprims > 1;
                const uint32_t kh = INST ? (oct >> 8) << kargs()->S.gBits : 0u;
                if constexpr (TRI) {   // (the triangle-only branch below, alone)
                    wideTestTri(q0, mL, o, d, 0.001f, closest, best, bestLo);
                    wideTestTri(q1, m1, o, d, 0.001f, closest, best, bestLo);
                    PT_COUNT(sTris, (uint32_t)nL + (uint32_t)__popcll(m1));
                } else if (kargs()->S.hasSpheres) {   // (uniform: read where needed)
                    if (h0) wideTest<true>(q0, o, d, inv, 0.001f, closest, best, bestLo, lb, redo, kh);
                    if (h1) wideTest<true>(q1, o, d, inv, 0.001f, closest, best, bestLo, lb, redo, kh);
                    const uint64_t s0 = mL & __ballot(__float_as_uint(q0.p2.w) != 0u);
                    const uint64_t s1 = m1 & __ballot(__float_as_uint(q1.p2.w) != 0u);
                    PT_COUNT(sTris, (uint32_t)nL + (uint32_t)__popcll(m1) - (uint32_t)__popcll(s0) - (uint32_t)__popcll(s1));
                    PT_COUNT(sSph, (uint32_t)__popcll(s0) + (uint32_t)__popcll(s1));
                } else {
                    if constexpr (INST) {
                        if (h0) wideTest<false>(q0, o, d, inv, 0.001f, closest, best, bestLo, lb, redo, kh);
                        if (h1) wideTest<false>(q1, o, d, inv, 0.001f, closest, best, bestLo, lb, redo, kh);
                    } else {   // the leaf-box rule is decided once, in SHADE (bestLo holds t2)
                        wideTestTri(q0, mL, o, d, 0.001f, closest, best, bestLo);
                        wideTestTri(q1, m1, o, d, 0.001f, closest, best, bestLo);
                    }
                    PT_COUNT(sTris, (uint32_t)nL + (uint32_t)__popcll(m1));
                }
                if (redo) oct |= 8u;   // order-dependent candidate: repeat the query in the reference's order
                if (SPEC && tg == 0u && (oct & 48u)) {   // this group is done: the last parked one is next
                    oct -= 16u;
                    const uint32_t c = SPECN == 1 ? 0u : (oct >> 4) & 3u;
                    tgBase = pend[(2u * c) * kWave + lane];
                    tg = pend[(2u * c + 1u) * kWave + lane];
#ifdef PT_DIAG
                    oct |= 64u;
#endif
                }
            } else {
            PT_DIAG_ADD(sPops, (uint32_t)nL);
            // Every lane tests all of its queued leaves, in order, in this step (the queue then
            // is empty and the lane rejoins NODE steps; measured -4 % vs one leaf per step).
            // The first two queued primitives are loaded together up front (their addresses are
            // known; only the tests depend on `closest`): one memory round trip for two leaves.
            Prim pf0{}, pf1{};
            if (qn > 0) pf0 = loadPrim(S, qref[0] & kPrimMask);
            if (qn > 1) pf1 = loadPrim(S, qref[1] & kPrimMask);
#pragma unroll
            for (int k_ = 0; k_ < LQ; k_++) {
                const bool act = qn > 0;
                if (__ballot(act) == 0) break;
                tested = false;
                sph = false;
            if (act) {
                const uint32_t ref = qref[0];
                const float lo = lq[0];
#pragma unroll
                for (int i = 0; i + 1 < LQ; i++) { qref[i] = qref[i + 1]; lq[i] = lq[i + 1]; }
                qn--;
                const uint32_t k = ref & kPrimMask;
                sph = (ref & kSphereBit) != 0;
                // Exact re-test of the leaf box with the current closest: the box passed when it
                // was queued, with a tmax >= closest, so now it fails iff closest < lo (slabLo).
                if (!(closest < lo)) {
                    const Prim pr = k_ == 0 ? pf0 : (k_ == 1 ? pf1 : loadPrim(S, k));
                    // (wide: a leaf that waited on the stack has no entry distance, lo = -inf:
                    // exact re-test of its box from the primitive's vertices)
                    {
                        tested = true;
                        const float t = primHitT(pr, sph, o, d, 0.001f, closest);
                        if (t >= 0.0f) { closest = t; best = (int)k; }
                    }
                }
            }
            PT_COUNT(sTris, (uint32_t)__popcll(__ballot(tested && !sph)));
            PT_COUNT(sSph, (uint32_t)__popcll(__ballot(tested && sph)));
            }
            }
        }
        if (kind == 2) {
            // ------------------------------------------------------------------ SHADE
            const uint64_t shadeM = mS & ~needTaskM;   // lanes whose query is complete
            const bool shading = laneOf(shadeM);
            // NEE: the lane's flags (a lane that is not shading reads stale ones; `shading` masks them)
            uint32_t nf = 0u;
            if constexpr (NEE) nf = neeF[lane];
            const bool shadowQ = NEE && (nf & 1u) != 0u;   // the finished query was a shadow ray
            if constexpr (WIDE && !INST) {
                bool redo = shading && (oct & 8u);
#ifdef PT_DIAG
                bool missed = false;
#endif
                // Triangle-only scenes: the reference's leaf-box rule, decided here for the final
                // hit alone (deferredRedo; bestLo holds t2)
                bool triScene = TRI;
                if constexpr (!TRI) triScene = !kargs()->S.hasSpheres;
                if (triScene && S.nprims > 1) {
                    if (shading && best >= 0 && !redo) {
                        // (a 32-bit byte offset: 32 best < 2^31, < 2^26 primitives)
                        const float4* bx = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(kargs()->S.wbox) +
                                                                           ((uint32_t)best << 5));
                        redo = deferredRedo(bx[0], *reinterpret_cast<const float2*>(bx + 1), o, inv, closest, bestLo);
#ifdef PT_DIAG
                        {   // (which of them because the ray misses the final hit's box outright)
                            const float2 bz_ = *reinterpret_cast<const float2*>(bx + 1);
                            const float4 bx_ = bx[0];
                            missed = !slabPair(v2f{bx_.x, bx_.y}, v2f{bx_.z, bx_.w}, v2f{bz_.x, bz_.y}, o, inv, 0.001f,
                                               __builtin_inff()).hit;
                        }
#endif
                    }
                }
                // rare: an order-dependent query (or a far origin), repeated in the reference's
                // order.  Ranks index wshade.
                PT_DIAG_ADD(sRedo, (uint32_t)__popcll(__ballot(redo)));
                PT_DIAG_ADD(sRedoMiss, (uint32_t)__popcll(__ballot(missed)));
                if (redo) {
                    const DevScene S2 = ldScene(kargs());
                    closest = shadowQ ? kShadowTmax : __builtin_inff();   // (the query's own start value)
                    const int k = traceRefStackless(S2, o, d, 0.001f, closest);
                    best = k >= 0 ? (int)S2.rankOf[k] : -1;
                }
            }
            PT_DIAG_ADD(itS, 1u);
#ifdef PT_DIAG
            uint32_t nTrials = 0u;   // the lane's trials of the unit-sphere loop in this step
#endif
            if constexpr (AHEAD) {
                // A. Classify.  A miss, an emitter or an absorbing type ends the sample; a Lambertian hit
                // scatters: att *= albedo, o = the hit point, and d holds the shading normal until D adds
                // the unit vector (the ray's old direction is dead once `front` is known).
                bool done = false;
                if (shading) {
                    float3 contrib = f3(0.0f, 0.0f, 0.0f);
                    done = true;
                    if (best < 0) {
                        contrib = PT_SKY();
                    } else {   // makeHitFrom's record, of which a Lambertian-only scene needs the normal, the albedo and the type
                        const float4* r = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(kargs()->S.wshade) +
                                                                          mul48((uint32_t)(best & (int)kPrimMask)));
                        const float4 s0 = r[0], s1 = r[1];
                        const uint32_t tf = __float_as_uint(r[2].y);
                        if ((tf & 0xffffu) == (uint32_t)PT_LAMBERTIAN) {
                            const float3 p = add(o, scale(closest, d));
                            float3 outward = xyz(s0);
                            if constexpr (!TRI) {
                                if (tf >> 16) outward = divs(sub(p, xyz(s0)), s0.w);   // sphere: (p - c) / r
                            }
                            const bool front = dot3(d, outward) < 0.0f;
                            o = p;
                            d = front ? outward : neg(outward);
                            att = mul(att, xyz(s1));
                            done = false;
                        } else if constexpr (LIT) {
                            if ((tf & 0xffffu) == (uint32_t)PT_EMISSIVE) contrib = mul(att, xyz(s1));
                        }
                    }
                    if (done) sum = add(sum, contrib);
                }
                // B. Step the sample, finish tasks, take tasks, new paths: before the loop, so that a fresh
                // path draws along at once.  Every shading lane either completed its sample or scatters.
                const uint4 ts = taskState[lane];
                const uint32_t y1 = ts.y + (done ? 1u : 0u);
                taskState[lane].y = y1;
                const uint64_t doneM = shadeM & __ballot(y1 != ts.y), finM = doneM & __ballot(y1 == ts.z);
                const uint64_t scM = shadeM & ~doneM;
                if (laneOf(finM)) PT_FINISH_TASK(ts);
                needTaskM |= finM;
                activeM &= ~finM;
                uint64_t newSampleM = doneM & ~finM, got = 0;
#ifdef PT_DIAG
                const unsigned long long tS1 = __builtin_amdgcn_s_memtime();
#endif
                PT_TAKE_TASKS(got);
                activeM |= got;
                newSampleM |= got;
#ifdef PT_DIAG
                const unsigned long long tS2 = __builtin_amdgcn_s_memtime();
#endif
                if (laneOf(newSampleM)) PT_NEW_PATH();
#ifdef PT_DIAG
                const unsigned long long tS3 = __builtin_amdgcn_s_memtime();
#endif
                haveM &= ~(doneM | got);   // (a re-seeded stream: the slot's vector belonged to the old one)
                // C. One trial loop.  pendM: scatter lanes without a vector -- the loop runs until each of
                // them has accepted, not at all when there is none.  Every other lane on a path with an
                // empty slot draws along (a scatter lane whose slot was full empties it in D, so it is one
                // of them).  A lane leaves at its first acceptance; per trial the wave adds scalar mask
                // operations only.
                const uint64_t pendM = scM & ~haveM, hadM = scM & haveM;
                haveM &= ~scM;
                const uint64_t drawM = activeM & ~haveM;
                float3 res = f3(0.0f, 0.0f, 0.0f);
                float norm = 2.0f;
                if (pendM != 0 && laneOf(drawM)) {
                    uint64_t waitM = pendM;
                    for (;;) {   // draws x, y, z in order, as onUnitSphere does
                        res = g.centered2x3();
                        norm = len2(res);
#ifdef PT_DIAG
                        nTrials++;
#endif
                        waitM &= ~__ballot(norm < 1.0f);
                        if (norm < 1.0f || waitM == 0) break;
                    }
                }
                // D. Slots, in this LDS order: a scatter lane that had a vector reads it; a lane that drew
                // along and accepted writes its own.  Then d = n + v / sqrt(len2(v)) with scatterInto's
                // degenerate-direction rule (len2 recomputed from the stored triple: the same bits).
                float3 held = f3(0.0f, 0.0f, 0.0f);
                if (laneOf(hadM)) held = f3(aheadV[0 * kWave + lane], aheadV[1 * kWave + lane], aheadV[2 * kWave + lane]);
                const uint64_t keepM = drawM & ~pendM & __ballot(norm < 1.0f);
                if (laneOf(keepM)) {
                    aheadV[0 * kWave + lane] = res.x; aheadV[1 * kWave + lane] = res.y; aheadV[2 * kWave + lane] = res.z;
                }
                haveM |= keepM;
                if (laneOf(scM)) {
                    const bool drew = laneOf(pendM);
                    const float3 v = f3(drew ? res.x : held.x, drew ? res.y : held.y, drew ? res.z : held.z);
                    const float3 dir = add(d, divs(v, sqrtf(len2(v))));
                    const bool tiny = fabsf(dir.x) < 1e-7f && fabsf(dir.y) < 1e-7f && fabsf(dir.z) < 1e-7f;
                    d = f3(tiny ? d.x : dir.x, tiny ? d.y : dir.y, tiny ? d.z : dir.z);
                }
                // A scatter at depthLeft == 0 begins no ray and is not counted: it stays in mS (tg, sp and
                // ng's child bits are 0 for every lane of shadeM) as a miss, and the next SHADE step's miss
                // branch gives it PT_SKY() of the scattered d and the multiplied att.
                const uint64_t lastM = scM & __ballot(depthLeft == 0);
                if (laneOf(lastM)) { best = -1; oct = 0u; }
                // E. Ray start for the lanes that go on.
                const uint64_t newRayM = ((shadeM & ~finM) | got) & ~lastM;
#ifdef PT_DIAG
                const unsigned long long tS4 = __builtin_amdgcn_s_memtime();
#endif
                if (laneOf(newRayM)) PT_BEGIN_RAY(false);
#ifdef PT_DIAG
                // (shading: steps A and B up to the tasks, and the trial loop with the slots, C and D)
                cycSh += (tS1 - tK0) + (tS4 - tS3); cycTk += tS2 - tS1; cycNp += tS3 - tS2;
                cycBr += __builtin_amdgcn_s_memtime() - tS4;
#endif
                PT_COUNT(sRays, (uint32_t)__popcll(newRayM));
                PT_COUNT(sPaths, (uint32_t)__popcll(newSampleM));
            } else {
                bool done = false;   // the lane's sample is complete
                bool shadowNow = false;   // NEE: the lane's next query is a shadow ray
                if (shading) {
                    float3 contrib = f3(0.0f, 0.0f, 0.0f);
                    bool wasShadow = false;
                    if constexpr (NEE) {
                        if (shadowQ) {   // the shadow query is complete: its term if nothing was hit, then the parked scatter ray
                            if (best < 0) {
                                neeV[0 * kWave + lane] += neeV[3 * kWave + lane];
                                neeV[1 * kWave + lane] += neeV[4 * kWave + lane];
                                neeV[2 * kWave + lane] += neeV[5 * kWave + lane];
                            }
                            d = f3(neeV[6 * kWave + lane], neeV[7 * kWave + lane], neeV[8 * kWave + lane]);
                            neeF[lane] = nf & ~1u;
                            wasShadow = true;
                        }
                    }
                    if (wasShadow) {
                    } else if (best < 0) {
                        contrib = PT_SKY();
                        done = true;
                    } else {
                        int objI_;
                        HitRec h = INST ? makeHitInst(ldScene(kargs()), (uint32_t)best & kPrimMask, closest, o, d, objI_)
                                        : (WIDE ? makeHitFrom<!TRI>(kargs()->S.wshade, best & (int)kPrimMask, closest, o, d)
                                                : makeHit(S, best, closest, o, d));
#ifdef PT_DIAG
                        if (!scatterInto(h, d, att, g, &nTrials)) {
#else
                        if (!scatterInto(h, d, att, g)) {
#endif
                            if constexpr (LIT) contrib = emitted(h, att);
                            if constexpr (NEE) {   // the light was sampled at the hit this ray left
                                // (instanced: the hit key's low gBits bits are the shading index)
                                const int sk = INST ? best & ((1 << kargs()->S.gBits) - 1) : best & (int)kPrimMask;
                                if ((nf & 2u) && sampledLight(kargs()->S.wshade, sk, h)) {
                                    if constexpr (MIS && INST)
                                        contrib = emittedWeightedAt(kargs()->lights,
                                                                    instLightSlot(kargs()->instLightFirst, kargs()->lightSlot,
                                                                                  (uint32_t)best & kPrimMask, kargs()->S.gBits),
                                                                    kargs()->nLights, closest, d, neeV[9 * kWave + lane], contrib);
                                    else if constexpr (MIS)
                                        contrib = emittedWeighted(kargs()->lights, kargs()->lightSlot, kargs()->nLights, h.obj,
                                                                  closest, d, neeV[9 * kWave + lane], contrib);
                                    else contrib = f3(0.0f, 0.0f, 0.0f);
                                }
                            }
                            done = true;
                        } else {
                            o = h.p;
                            if (depthLeft == 0) { contrib = PT_SKY(); done = true; }
                            else if constexpr (NEE) {
                                nf &= ~2u;
                                if (h.type == PT_LAMBERTIAN) {
                                    nf |= 2u;
                                    float3 w, term;
                                    if constexpr (MIS) neeV[9 * kWave + lane] = scatterPdf(h.n, d);
                                    if (lightSample<MIS>(kargs()->lights, kargs()->nLights, o, h.n, att, g, w, term)) {
                                        neeV[3 * kWave + lane] = term.x; neeV[4 * kWave + lane] = term.y; neeV[5 * kWave + lane] = term.z;
                                        neeV[6 * kWave + lane] = d.x; neeV[7 * kWave + lane] = d.y; neeV[8 * kWave + lane] = d.z;
                                        d = w;
                                        nf |= 1u;
                                        shadowNow = true;
                                    }
                                }
                                neeF[lane] = nf;
                            }
                        }
                    }
                    if (done) {
                        if constexpr (NEE)
                            contrib = neeTotal(f3(neeV[0 * kWave + lane], neeV[1 * kWave + lane], neeV[2 * kWave + lane]), contrib);
                        sum = add(sum, contrib);
                    }
                }
                // Every lane steps its sample count by `done` (a lane that is not shading by 0; shadeM
                // masks its stale state): who completed a sample and who its last one comes from two
                // integer compares, not from predicates joined over the branches above.
                uint64_t doneM, finM;
                if constexpr (SAMPLE) {
                    const uint4 ts = taskState[lane];
                    const uint32_t y1 = ts.y + (done ? 1u : 0u);
                    taskState[lane].y = y1;
                    doneM = shadeM & __ballot(y1 != ts.y);
                    finM = doneM & __ballot(y1 == ts.z);
                    if (laneOf(finM)) PT_FINISH_TASK(ts);
                    needTaskM |= finM;
                } else {
                    const int s1 = sample + (done ? 1 : 0);
                    doneM = shadeM & __ballot(s1 != sample);
                    finM = doneM & __ballot(s1 == nSamples);
                    sample = s1;
                }
                activeM &= ~finM;
                // bounce or next sample (newSampleM) for the lanes that go on
                uint64_t newRayM = shadeM & ~finM, newSampleM = doneM & ~finM;
#ifdef PT_DIAG
                const unsigned long long tS1 = __builtin_amdgcn_s_memtime();
#endif
                if constexpr (SAMPLE) {   // idle lanes take new tasks and start their first path
                    uint64_t got = 0;
                    PT_TAKE_TASKS(got);
                    activeM |= got;
                    newRayM |= got;
                    newSampleM |= got;
                }
                // one camera-ray and one ray-start site for every lane that needs them
#ifdef PT_DIAG
                const unsigned long long tS2 = __builtin_amdgcn_s_memtime();
#endif
                if (laneOf(newSampleM)) PT_NEW_PATH();
#ifdef PT_DIAG
                const unsigned long long tS3 = __builtin_amdgcn_s_memtime();
#endif
                if (laneOf(newRayM)) PT_BEGIN_RAY(shadowNow);
#ifdef PT_DIAG
                const unsigned long long tS4 = __builtin_amdgcn_s_memtime();
                cycSh += tS1 - tK0; cycTk += tS2 - tS1; cycNp += tS3 - tS2; cycBr += tS4 - tS3;
#endif
                PT_COUNT(sRays, (uint32_t)__popcll(newRayM));
                PT_COUNT(sPaths, (uint32_t)__popcll(newSampleM));
            }
#ifdef PT_DIAG
            // the step's trial-loop iterations: the wave repeats the trial as often as its slowest lane
            for (int w_ = 32; w_ > 0; w_ >>= 1) nTrials = max(nTrials, (uint32_t)__shfl_xor((int)nTrials, w_));
            sTrials += nTrials;
#endif
        }
#ifdef PT_DIAG
        {   // shader-clock cycles per step kind (the step's memory waits included)
            const unsigned long long dK = __builtin_amdgcn_s_memtime() - tK0;
            if (kind == 0) cycN += dK;
            else if (kind == 1) cycL += dK;
            else cycS += dK;
        }
#endif
    }
    if constexpr (!SAMPLE) {   // (sample mode: every task wrote its result when it ended)
        if (valid) {
            storePixel(P, idx, sum);
            P.sd[idx] = g.d; P.s0[idx] = g.v0; P.s1[idx] = g.v1; P.s2[idx] = g.v2; P.s3[idx] = g.v3; P.s4[idx] = g.v4;
            if (CRITK && P.pixRays) P.pixRays[idx] = pxRays;   // (the next launch's critical pixels)
        }
    }
    const unsigned long long tEnd = __builtin_amdgcn_s_memrealtime();
    if (!SAMPLE && !crit && lane == 0) atomicMax(P.tileCost + tile, (unsigned)min(tEnd - tStart, 0xffffffffull));   // (split tiles: several waves)
    if (P.waveTimes && lane == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        P.waveTimes[3 * (size_t)blockIdx.x + 0] = tStart;
        P.waveTimes[3 * (size_t)blockIdx.x + 1] = tEnd;
        P.waveTimes[3 * (size_t)blockIdx.x + 2] = (unsigned long long)tile | ((unsigned long long)(xcc & 0xf) << 32);
    }
    if (lane == 0) {
        atomicAdd(P.counters + 0, (unsigned long long)sRays);
        atomicAdd(P.counters + 1, (unsigned long long)sVisits);
        atomicAdd(P.counters + 2, (unsigned long long)sTris);
        atomicAdd(P.counters + 3, (unsigned long long)sSph);
        atomicAdd(P.counters + 4, (unsigned long long)sPaths);
#ifdef PT_DIAG
        atomicAdd(P.counters + 8, (unsigned long long)itN);
        atomicAdd(P.counters + 9, (unsigned long long)itL);
        atomicAdd(P.counters + 10, (unsigned long long)itS);
        atomicAdd(P.counters + 11, (unsigned long long)sPops);
        atomicAdd(P.counters + 12, cycN);
        atomicAdd(P.counters + 13, cycL);
        atomicAdd(P.counters + 14, cycS);
        atomicAdd(P.counters + 15, cycH);
        atomicAdd(P.counters + 16, cycSh);
        atomicAdd(P.counters + 17, cycTk);
        atomicAdd(P.counters + 18, cycNp);
        atomicAdd(P.counters + 19, cycBr);
        atomicAdd(P.counters + 20, (unsigned long long)sRedo);
        atomicAdd(P.counters + 21, sSpecN);
        atomicAdd(P.counters + 22, sIdleN);
        atomicAdd(P.counters + 23, (unsigned long long)sRedoMiss);
        atomicAdd(P.counters + 25, sHalf);
        atomicAdd(P.counters + 26, sTrials);
        atomicAdd(P.counters + 27, sParkT);
#endif
    }
}
#undef PT_BEGIN_RAY
#undef PT_CRIT_TRACE
#undef PT_NEW_PATH
#undef PT_SKY
#undef PT_TAKE_TASKS
#undef PT_FINISH_TASK
#undef PT_DIAG_ADD
#undef PT_COUNT

// Every render launch goes through these two macros (in scope: RenderParams P, hipStream_t st).
// PT_KERNEL_LOG not 0: the launch site names the instantiation it takes, one line on stderr per launch
// (host code; the template arguments are those of the launch itself, written out in full).
inline bool kernelLogOn() {
    const char* v = std::getenv("PT_KERNEL_LOG");
    return v && std::atoi(v) != 0;
}
inline const char* tf(bool b) { return b ? "true" : "false"; }
template <int STACK, bool SAMPLE, bool WIDE, bool INST = false, bool LIT = false, bool NEE = false, bool MIS = false,
          bool TRI = false, bool AHEAD = false>
inline void logLaunchWF() {
    if (kernelLogOn())
        std::fprintf(stderr, "[pt] kernel renderKernelWF<%d, %s, %s, %s, %s, %s, %s, %s, %s>\n", STACK, tf(SAMPLE), tf(WIDE),
                     tf(INST), tf(LIT), tf(NEE), tf(MIS), tf(TRI), tf(AHEAD));
}
template <int STACK, bool SAMPLE, bool LIT = false, bool NEE = false, bool MIS = false>
inline void logLaunchSimple() {
    if (kernelLogOn())
        std::fprintf(stderr, "[pt] kernel renderKernel<%d, %s, %s, %s, %s>\n", STACK, tf(SAMPLE), tf(LIT), tf(NEE), tf(MIS));
}
#define PT_LAUNCH_WF(grid, ...)                                                                     \
    do {                                                                                          \
        logLaunchWF<__VA_ARGS__>();                                                               \
        renderKernelWF<__VA_ARGS__><<<(grid), kWave, 0, st>>>(P);                                 \
    } while (0)
#define PT_LAUNCH_SIMPLE(grid, ...)                                                                 \
    do {                                                                                          \
        logLaunchSimple<__VA_ARGS__>();                                                           \
        renderKernel<__VA_ARGS__><<<(grid), kWave, 0, st>>>(P);                                   \
    } while (0)

#ifdef PT_TU_COMPAT
}  // namespace

// pt_compat.hip compiles this file a second time with PT_TU_COMPAT: only the device code above and
// this launcher of the compat-mode wide kernels (renderKernelWF<S, false, true>), built WITHOUT the
// -mllvm --enable-post-misched=0 of the main translation unit.  That flag speeds the sample-mode
// kernels up but slows the compat kernel -- one sequential chain of samples per pixel -- by 3.5 %
// (DESIGN.md section 6), and it is a per-file option.
namespace pt {
// TRI = P.tri: the triangle-only instantiations (critical-pixel waves included)
template <int S, bool TRI>
static void launchCompatWideTri(const RenderParams& P, hipStream_t st) {
    const int grid = P.compatGrid;
    if (P.nLights > 0 && P.mis) PT_LAUNCH_WF(grid, S, false, true, false, true, true, true, TRI);
    else if (P.nLights > 0) PT_LAUNCH_WF(grid, S, false, true, false, true, true, false, TRI);
    else if (P.lit) PT_LAUNCH_WF(grid, S, false, true, false, true, false, false, TRI);
    else PT_LAUNCH_WF(grid, S, false, true, false, false, false, false, TRI);
}
int launchCompatWide(int stack, const void* params, hipStream_t st) {
    const RenderParams& P = *static_cast<const RenderParams*>(params);
    switch (stack) {
#define PT_COMPAT_WIDE(S)                                                                    \
        case S:                                                                                  \
            P.tri ? launchCompatWideTri<S, true>(P, st) : launchCompatWideTri<S, false>(P, st);   \
            break;
        PT_COMPAT_WIDE(8)
        PT_COMPAT_WIDE(16)
        PT_COMPAT_WIDE(24)
#undef PT_COMPAT_WIDE
        default: return -1;
    }
    return 0;
}
template <bool TRI>
static const void* compatWideKernel(int stack) {
    return stack == 8 ? reinterpret_cast<const void*>(&renderKernelWF<8, false, true, false, false, false, false, TRI>)
         : stack == 16 ? reinterpret_cast<const void*>(&renderKernelWF<16, false, true, false, false, false, false, TRI>)
         : stack == 24 ? reinterpret_cast<const void*>(&renderKernelWF<24, false, true, false, false, false, false, TRI>) : nullptr;
}
int compatWideWavesPerCU(int stack, bool tri, int& n) {
    const void* k = tri ? compatWideKernel<true>(stack) : compatWideKernel<false>(stack);
    if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, kWave, 0) != hipSuccess) return -1;
    return 0;
}
}  // namespace pt
#else

// Frame epilogue (one lane per pixel).  The frame's linear sum S is the raw compat sum
// (`nblocks` = 0) or, in sample mode, the block sums added in order.  Accumulating films keep
// A += S over frames (progressive rendering, the headless counterpart of the reference's
// interactive loop, main.cu:489-528) and resolve sqrt(A * (1 / samples so far)); otherwise
// sqrt(S * (1 / spp)) (main.cu:290-293).  Output: fp32 RGB, or 8-bit RGBA quantised like
// PngImage::saveColor (png_image.h:24-30: (uint8)(clamp(c, 0, 0.999) * 256), alpha 255) or like
// renderBySurface (main.cu:327-331: (unsigned)(c * 255) into an 8-bit field, alpha 255).
// Rows stay in film order (row 0 = bottom); the PNG writer flips them.
// Sample mode: the pixel's 32-B accumulator {x, y, z (32.32 fixed point), rays}; its rays are
// added to its tile's cost (the next launch's longest-first order).
__global__ __launch_bounds__(256) void resolveKernel(const float* __restrict__ src,
                                                     const unsigned long long* __restrict__ pixAcc, float* accum,
                                                     float inv, int format, void* out, int64_t npix,
                                                     unsigned* tileCost, int width, int tilesX, int costMax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float x, y, z;
    if (!pixAcc) {
        x = src[3 * i + 0]; y = src[3 * i + 1]; z = src[3 * i + 2];
    } else {
        const ulonglong2* a2 = reinterpret_cast<const ulonglong2*>(pixAcc + 4 * i);
        const ulonglong2 a = a2[0], b = a2[1];
        x = fixedToFloat(a.x);
        y = fixedToFloat(a.y);
        z = fixedToFloat(b.x);
        const uint32_t rays = (uint32_t)min(b.y, 0xffffffffull);
        if (tileCost) {
            const int row = (int)(i / width), col = (int)(i - (int64_t)row * width);
            unsigned* tc = tileCost + (row >> 3) * tilesX + (col >> 3);
            if (costMax) atomicMax(tc, rays);
            else atomicAdd(tc, rays);
        }
    }
    if (accum) {
        float* a = accum + 3 * i;
        x = a[0] + x; y = a[1] + y; z = a[2] + z;
        a[0] = x; a[1] = y; a[2] = z;
    }
    const float c[3] = {sqrtf(x * inv), sqrtf(y * inv), sqrtf(z * inv)};
    if (format == PT_OUT_RGB32F) {
        float* o = static_cast<float*>(out) + 3 * i;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
        return;
    }
    uint32_t px = 0xff000000u;
    for (int k = 0; k < 3; k++) {
        uint32_t b;
        if (format == PT_OUT_RGBA8) {
            float v = c[k];                  // utility.h:40-44 clamp(x, 0, 0.999f), then * 256
            if (v < 0.0f) v = 0.0f;
            if (v > 0.999f) v = 0.999f;
            b = (uint32_t)(v * 256.0f);
        } else {
            b = (uint32_t)(c[k] * 255.0f) & 0xffu;
        }
        px |= b << (8 * k);
    }
    static_cast<uint32_t*>(out)[i] = px;
}

// Longest-first launch order on the device: keys ~cost (ascending = cost descending) and tile ids,
// then a stable radix sort (pt_sort.hip): equal costs keep ascending tile ids.
// Sample mode: each launch slot's tile as tx | ty << 16 (`order` = the longest-first launch order,
// null = identity), so the task hand-out does no divisions per take.
__global__ __launch_bounds__(256) void tileXYKernel(const uint32_t* __restrict__ order, int n, int tilesX, uint32_t* xy) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = order ? order[i] : (uint32_t)i;
    const uint32_t ty = t / (uint32_t)tilesX;
    xy[i] = (t - ty * (uint32_t)tilesX) | (ty << 16);
}

// compat: mark the next launch's critical pixels (the first k of the pixels sorted by rays)
__global__ __launch_bounds__(256) void critFlagKernel(const uint32_t* __restrict__ sorted, int k, uint8_t* flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) flag[sorted[i]] = 1;
}

__global__ __launch_bounds__(256) void tileKeyKernel(const unsigned* __restrict__ cost, uint32_t* keys, uint32_t* ids,
                                                     int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ~cost[i];
    ids[i] = (uint32_t)i;
}

// ------------------------------------------------------------------------ ray queries
// Six query kernels: closest hit on the binary tree (traceKernel, queued: traceKernelQ) and on the
// wide tree (traceKernelWide, traceKernelWideQ), any hit on either tree (occludedKernelQ,
// occludedKernelWideQ).  Each is a composition of the pieces below, which exist once: the hit
// records, the binary tree's query start and node visit (binStart, binVisit), the wide walk's
// query start, closest-hit primitive group and node step (wideStart, wideGroupClosest, wideStep).

__device__ __forceinline__ void flushCounters(unsigned long long* counters, const Counters& c) {
    waveReduceAdd(counters + 0, c.rays);
    waveReduceAdd(counters + 1, c.visits);
    waveReduceAdd(counters + 2, c.tris);
    waveReduceAdd(counters + 3, c.spheres);
}

__device__ __forceinline__ pt_hit missRecord() {
    pt_hit h = {};
    h.obj = -1;
    h.mat = -1;
    return h;
}
__device__ __forceinline__ pt_hit hitRecord(const HitRec& x, float t) {
    pt_hit h = missRecord();
    h.hit = 1;
    h.obj = x.obj;
    h.mat = x.mat;
    h.front_face = x.front ? 1 : 0;
    h.t = t;
    h.p[0] = x.p.x; h.p[1] = x.p.y; h.p[2] = x.p.z;
    h.n[0] = x.n.x; h.n[1] = x.n.y; h.n[2] = x.n.z;
    return h;
}
// The binary tree's record: leaf slot k (< 0: a miss) at distance t.
__device__ __forceinline__ pt_hit binHit(const DevScene& S, int k, float t, float3 o, float3 d) {
    return k >= 0 ? hitRecord(makeHit(S, k, t, o, d), t) : missRecord();
}

// One primitive test of a fixed interval (any hit), counted as primTest counts it.
__device__ __forceinline__ bool primTestAny(const DevScene& S, uint32_t ref, float3 o, float3 d, float tmin, float tmax,
                                            Counters& c) {
    const bool sph = (ref & kSphereBit) != 0;
    if (sph) c.spheres++;
    else c.tris++;
    return primHitT(loadPrim(S, ref & kPrimMask), sph, o, d, tmin, tmax) >= 0.0f;
}

// A lane's walk of the binary tree in the reference's order (trace<STACK>), one node visit at a
// time.  `hi` is the interval's upper bound: closest hit shrinks it to the nearest hit so far and
// keeps that leaf in `best`; ANY keeps it fixed and stops at the first accepted primitive, with
// best = 0 for "hit" (-1: none).
struct BinWalk {
    float3 o, d, inv;
    int node, sp, guard;
};
template <bool ANY>
__device__ __forceinline__ bool binLeaf(const DevScene& S, uint32_t ref, const BinWalk& w, float tmin, float& hi,
                                        int& best, Counters& c) {   // true: the walk ends here
    if constexpr (ANY) {
        const bool hit = primTestAny(S, ref, w.o, w.d, tmin, hi, c);
        best = hit ? 0 : -1;
        return hit;
    } else {
        primTest(S, ref, w.o, w.d, tmin, hi, best, c);
        return false;
    }
}
// The query's start; true: it is already answered (no tree to walk).
template <bool ANY>
__device__ __forceinline__ bool binStart(const DevScene& S, pt_ray r, float tmin, float tmax, BinWalk& w, float& hi,
                                         int& best, Counters& c) {
    w.o = f3(r.o[0], r.o[1], r.o[2]);
    w.d = f3(r.d[0], r.d[1], r.d[2]);
    hi = tmax;
    best = -1;
    c.rays++;
    if (S.nprims <= 1) {
        if (S.nprims == 1)   // root is a leaf: tested without a box test (:92-98)
            binLeaf<ANY>(S, kLeafBit | (__float_as_uint(S.prims[2].w) ? kSphereBit : 0u), w, tmin, hi, best, c);
        return true;
    }
    w.inv = f3(rcpRN(w.d.x), rcpRN(w.d.y), rcpRN(w.d.z));
    w.node = 0;
    w.sp = 0;
    w.guard = 0;
    return false;
}
// One node visit: both children's slab tests, a leaf child tested at once, an internal child
// pushed (left, then right), then the pop.  true: the walk ended.
template <int STACK, bool ANY>
__device__ __forceinline__ bool binVisit(const DevScene& S, uint32_t* my, float tmin, BinWalk& w, float& hi, int& best,
                                         Counters& c) {
    if (++w.guard > S.nprims) { atomicOr(S.err, 1u); return true; }   // (a corrupt tree, trace<STACK>)
    c.visits++;
    const float4* np = S.nodes + 4 * (size_t)w.node;
    const float4 a = np[0], b = np[1], q = np[2], rr = np[3];
    const uint32_t lref = __float_as_uint(rr.x), rref = __float_as_uint(rr.y);   // (read here: one 16-B load)
    const auto child = [&](uint32_t ref) {   // a child whose box passed
        if (ref & kLeafBit) return binLeaf<ANY>(S, ref, w, tmin, hi, best, c);
        if (w.sp < STACK) { my[w.sp * kWave] = ref; w.sp++; return false; }
        atomicOr(S.err, 2u);
        return true;
    };
    if (slabLeft(a, b, w.o, w.inv, tmin, hi).hit && child(lref)) return true;
    if (slabRight(b, q, w.o, w.inv, tmin, hi).hit && child(rref)) return true;
    if (w.sp == 0) return true;
    w.sp--;
    w.node = (int)my[w.sp * kWave];
    return false;
}

// A lane's walk of the wide tree: the same traversal as renderKernelWF's WIDE steps, one lane per
// ray.  INST: an instanced scene's two-level tree (renderKernelWF<.., INST>).
struct WideWalk {
    float3 wo2, wd, winv;   // the world ray (instanced, far origin: moved to its entry into the world)
    float3 o, d, inv;       // the ray walked (inside an instance: in its object space)
    uint32_t woct, oct, inst;  // inst: the instance entered (read by the closest-hit kernels only)
    uint32_t ng, tgBase, tg;   // the node's remaining children; the primitive group to test
    float shift, tminI;        // (tmin, tmax of the moved ray: t - shift)
    int sp;
    uint32_t visits;   // the query's node visits: read by traceKernelWideQ under PT_TRACE_DIAG_VISITS only, else dead
};
// The query's start: the walk's state and `hi`, the interval's (shifted) upper bound.  true: a far
// origin, a direction the MIX planes cannot take, or a scene of one primitive; the walk is empty and
// the caller answers the query in the reference's order.
template <bool INST>
__device__ __forceinline__ bool wideStart(const DevScene& S, pt_ray r, float tmin, float tmax, WideWalk& w, float& hi,
                                          Counters& c) {
    const float3 wo = f3(r.o[0], r.o[1], r.o[2]);
    w.wd = f3(r.d[0], r.d[1], r.d[2]);
    w.winv = f3(rcpRN(w.wd.x), rcpRN(w.wd.y), rcpRN(w.wd.z));
    w.woct = (w.winv.x < 0.0f ? 1u : 0u) | (w.winv.y < 0.0f ? 2u : 0u) | (w.winv.z < 0.0f ? 4u : 0u);
    w.o = wo; w.d = w.wd; w.inv = w.winv;
    w.oct = w.woct;
    w.inst = 0u;
    // (a single primitive is the reference's root: tested with no box test at all (:92-98), so a hit its
    // arithmetic reports outside the primitive's box -- t = +inf from an overflowing direction, say --
    // counts; the wide root's box test would drop it, the reference-order query has none)
    const bool far = !INST && (S.nprims == 1 || wideFar(S, w.o) || (PT_WIDE_MIX && mixUnsafe(w.winv, S.mixLim)));
    // instanced: a far origin moves to the ray's entry into the world (instEntry); distances
    // are then measured from there and shifted back at the end
    w.wo2 = wo;
    w.shift = (INST && instFar(S, wo)) ? instEntry(S.cx, S.cy, S.cz, S.ext, w.wo2, w.wd, w.winv) : 0.0f;
    if (INST) w.o = w.wo2;
    w.tminI = tmin - w.shift;
    hi = tmax - w.shift;
    w.sp = 0;
    w.ng = S.nprims > 0 && !far ? (1u << w.oct) : 0u;
    w.tgBase = 0u;
    w.tg = 0u;
    w.visits = 0u;
    c.rays++;
    return far;
}
// One step after the lane's primitive group: pop (a marker returns to the world ray), the nearest
// remaining child, the rest pushed, the node's load, then the instance's entry or the node test
// over [tminI, hi].  true: the walk ended (or overflowed its stack, flagged).
template <int STACK, bool INST>
__device__ __forceinline__ bool wideStep(const DevScene& S, __amdgpu_buffer_rsrc_t nodeRsrc, uint32_t* my, float hi,
                                         WideWalk& w, Counters& c) {
    if constexpr (INST) {
        while ((w.ng & 0xffu) == 0u && w.sp > 0) {
            w.sp--;
            w.ng = my[w.sp * kWave];
            if (w.ng == kInstMarker) { w.o = w.wo2; w.d = w.wd; w.inv = w.winv; w.oct = w.woct; w.ng = 0u; }
        }
        if ((w.ng & 0xffu) == 0u) return true;
    } else if ((w.ng & 0xffu) == 0u) {
        if (w.sp == 0) return true;
        w.sp--;
        w.ng = my[w.sp * kWave];
    }
    const uint32_t bit = (uint32_t)__builtin_ctz(w.ng & 0xffu);
    const uint32_t child = (w.ng >> 8) + (bit ^ w.oct);
    w.ng &= ~(1u << bit);
    if (w.ng & 0xffu) {
        if (w.sp >= STACK) { atomicOr(S.err, 2u); return true; }
        my[w.sp * kWave] = w.ng;
        w.sp++;
    }
    c.visits++;
    w.visits++;
    const uint32_t off = mul80(child);
    const uint4 n0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off, 0, 0));
    const uint4 n1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 16u, 0, 0));
    const uint4 n2 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 32u, 0, 0));
    const uint4 n3 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 48u, 0, 0));
    const uint4 n4 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(nodeRsrc, off + 64u, 0, 0));
    if (INST && n0.w == kInstFlag) {   // an instance: into its object space and bottom-level tree
        if (n0.x == 0u) {
            const float4 r0 = __builtin_bit_cast(float4, n2), r1 = __builtin_bit_cast(float4, n3),
                         r2 = __builtin_bit_cast(float4, n4);
            w.o = xformPoint(r0, r1, r2, w.wo2);
            w.d = xformDir(r0, r1, r2, w.wd);
            w.inv = f3(rcpRN(w.d.x), rcpRN(w.d.y), rcpRN(w.d.z));
            w.oct = (w.inv.x < 0.0f ? 1u : 0u) | (w.inv.y < 0.0f ? 2u : 0u) | (w.inv.z < 0.0f ? 4u : 0u);
        }
        if (w.sp >= STACK) { atomicOr(S.err, 2u); return true; }
        my[w.sp * kWave] = kInstMarker;
        w.sp++;
        w.ng = (n1.x << 8) | (1u << w.oct);
        w.inst = n1.y;
        w.tg = 0u;
        return false;
    }
    const uint32_t h = INST ? wideHitsInst(n0, n1, n2, n3, n4, w.o, w.inv, w.oct, w.tminI, hi)
                            : wideHits<PT_WIDE_MIX != 0>(n0, n1, n2, n3, n4, w.o, w.inv, w.oct, w.tminI, hi);
    w.ng = (n1.x << 8) | (h >> 24);
    w.tgBase = n1.y;
    w.tg = h & 0xffffffu;
    return false;
}

// The closest-hit walk's result so far (wideTest): `redo` = an order-dependent candidate, the query
// is answered in the reference's order at the end.
struct WideBest {
    float closest, bestLo;
    int best;
    bool redo;
};
template <bool INST>
__device__ __forceinline__ void wideStartClosest(const DevScene& S, pt_ray r, float tmin, float tmax, WideWalk& w,
                                                 WideBest& b, Counters& c) {
    b.redo = wideStart<INST>(S, r, tmin, tmax, w, b.closest, c);
    b.best = -1;
    b.bestLo = -__builtin_inff();
}
// The closest-hit tests of the lane's primitive group.
template <bool INST>
__device__ __forceinline__ void wideGroupClosest(const DevScene& S, WideWalk& w, WideBest& b, Counters& c) {
    while (w.tg) {
        const uint32_t k = w.tgBase + (uint32_t)__builtin_ctz(w.tg);
        w.tg &= w.tg - 1u;
        const float4* p = S.wprims + 3 * (size_t)k;
        const Prim q{p[0], p[1], p[2]};
        if (__float_as_uint(q.p2.w) != 0u) c.spheres++;
        else c.tris++;
        const bool lb = !INST && S.nprims > 1;
        const uint32_t kh = INST ? w.inst << S.gBits : 0u;
        if (S.hasSpheres) wideTest<true>(q, w.o, w.d, w.inv, w.tminI, b.closest, b.best, b.bestLo, lb, b.redo, kh);
        else wideTest<false>(q, w.o, w.d, w.inv, w.tminI, b.closest, b.best, b.bestLo, lb, b.redo, kh);
    }
}
// The finished walk's hit: false for a miss, else the shading record x and the distance t along the
// query's ray (what the trace kernels report, what the AOV kernel reads the material from).
template <bool INST>
__device__ __forceinline__ bool wideHitRec(const DevScene& S, const WideWalk& w, WideBest& b, float tmin, float tmax,
                                           HitRec& x, float& t) {
    if (b.redo) {   // an order-dependent candidate: the query in the reference's order
        b.closest = tmax;
        const int k = traceRefStackless(S, w.o, w.d, tmin, b.closest);
        b.best = k >= 0 ? (int)S.rankOf[k] : -1;
    }
    if (b.best < 0) return false;
    int obj = 0;
    x = INST ? makeHitInst(S, (uint32_t)b.best & kPrimMask, b.closest, w.wo2, w.wd, obj)
             : makeHitFrom(S.wshade, b.best & (int)kPrimMask, b.closest, w.o, w.d);
    t = INST ? b.closest + w.shift : b.closest;
    return true;
}
// The finished walk's record, the same as traceKernel's.
template <bool INST>
__device__ __forceinline__ pt_hit wideHit(const DevScene& S, const WideWalk& w, WideBest& b, float tmin, float tmax) {
    HitRec x;
    float t;
    return wideHitRec<INST>(S, w, b, tmin, tmax, x, t) ? hitRecord(x, t) : missRecord();
}

// pt_trace_closest on the binary LBVH, in the reference order (trace<STACK>).
template <int STACK>
__global__ __launch_bounds__(kWave) void traceKernel(DevScene S, const pt_ray* rays, int64_t n, float tmin,
                                                     float tmax, pt_hit* hits, unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    Counters c{0, 0, 0, 0};
    // grid-stride over the batch: the counters are summed once per wave at the end (one global
    // atomic per counter per wave of a 64-ray block was the bottleneck of large batches)
    for (int64_t base = (int64_t)blockIdx.x * kWave; base < n; base += (int64_t)gridDim.x * kWave) {
    const int64_t i = base + lane;
    if (i < n) {
        const pt_ray r = rays[i];
        const float3 o = f3(r.o[0], r.o[1], r.o[2]), d = f3(r.d[0], r.d[1], r.d[2]);
        float closest = tmax;
        c.rays++;
        const int k = trace<STACK>(S, o, d, tmin, closest, stk + lane, c);
        hits[i] = binHit(S, k, closest, o, d);
    }
    }
    flushCounters(counters, c);
}

// pt_trace_closest on the wide tree (PT_KERNEL_WIDE), the same hit records as traceKernel.
template <int STACK, bool INST>
__global__ __launch_bounds__(kWave) void traceKernelWide(DevScene S, const pt_ray* rays, int64_t n, float tmin,
                                                         float tmax, pt_hit* hits, unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    const __amdgpu_buffer_rsrc_t nodeRsrc = rawRsrc(S.wnodes);
    Counters c{0, 0, 0, 0};
    for (int64_t base = (int64_t)blockIdx.x * kWave; base < n; base += (int64_t)gridDim.x * kWave) {   // grid-stride
    const int64_t i = base + lane;
    if (i < n) {
        WideWalk w;
        WideBest b;
        wideStartClosest<INST>(S, rays[i], tmin, tmax, w, b, c);
        do wideGroupClosest<INST>(S, w, b, c);
        while (!wideStep<STACK, INST>(S, nodeRsrc, my, b.closest, w, c));
        hits[i] = wideHit<INST>(S, w, b, tmin, tmax);
    }
    }
    flushCounters(counters, c);
}

// Queued closest-hit kernels (the default for pt_trace_closest; PT_TRACE_STRIDE=1 selects the
// grid-stride kernels above).  Persistent waves with a wave-level ray queue (Aila & Laine 2009,
// "persistent while-while" with dynamic fetch): a lane whose ray has finished takes the next
// ray of the batch at the top of the next loop iteration instead of idling until the wave's
// slowest ray is done.  The lanes that ask are ranked by a ballot and an mbcnt prefix count and
// served, in lane order, from the wave's pool of kTraceGrab consecutive rays (one returning
// atomic per pool on a queue word of the scene's counters).  Each loop iteration runs one
// traversal step per lane -- the reference order's node visit with its leaf tests (binVisit),
// or the wide tree's primitive group + next node (wideGroupClosest, wideStep) -- the very code
// of the grid-stride kernels, so every hit record and work counter is the same.
#ifndef PT_TRACE_GRAB
#define PT_TRACE_GRAB 256   // rays per queue grab (a wave's pool)
#endif
constexpr uint32_t kTraceGrab = PT_TRACE_GRAB;
#ifndef PT_TRACE_DIAG_REDO
#define PT_TRACE_DIAG_REDO 0   // diagnostic builds: count the queries that take the reference-order redo as sphere tests
#endif
#ifndef PT_TRACE_DIAG_VISITS
#define PT_TRACE_DIAG_VISITS 0   // diagnostic builds: each hit record's `mat` = the query's wide node visits
#endif
#ifndef PT_TRACE_WAVES
#define PT_TRACE_WAVES 1   // occupancy target of the queued trace kernels (waves per SIMD; 1 = the compiler's choice)
#endif
constexpr int kTraceQueue = 24;   // counters[24]: the ray queue (zeroed with the counters before each trace)

// Hand rays to the lanes that have none (`ray` < 0): ballot of the askers, each asker's rank among
// them (mbcnt), one pool refill by the first asker when the pool is empty.  poolBase / poolLeft /
// more are wave-uniform; `took` is set for a lane that received ray `ray` (< n).
#define PT_TRACE_REFILL(took)                                                                       \
    do {                                                                                          \
        for (;;) {                                                                                \
            const uint64_t m_ = __ballot(ray < 0 && more);                                        \
            if (m_ == 0) break;                                                                   \
            if (poolLeft == 0u) {                                                                 \
                const int leader_ = __ffsll((unsigned long long)m_) - 1;                          \
                unsigned long long b_ = 0;                                                        \
                if (lane == leader_) b_ = atomicAdd(counters + kTraceQueue, (unsigned long long)kTraceGrab); \
                const uint32_t lo_ = (uint32_t)__shfl((int)(uint32_t)b_, leader_);                \
                const uint32_t hi_ = (uint32_t)__shfl((int)(uint32_t)(b_ >> 32), leader_);         \
                poolBase = (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane(hi_) << 32) |       \
                                     __builtin_amdgcn_readfirstlane(lo_));                        \
                poolLeft = kTraceGrab;                                                            \
                if (poolBase >= n) { more = false; break; }                                       \
            }                                                                                     \
            const uint32_t take_ = min((uint32_t)__popcll(m_), poolLeft);                         \
            const uint32_t k_ = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m_ >> 32),         \
                                    __builtin_amdgcn_mbcnt_lo((uint32_t)m_, 0u));                 \
            if (ray < 0 && k_ < take_ && poolBase + (int64_t)k_ < n) {                            \
                ray = poolBase + (int64_t)k_;                                                     \
                took = true;                                                                      \
            }                                                                                     \
            poolBase += take_;                                                                    \
            poolLeft -= take_;                                                                    \
            if (poolBase >= n) more = false;                                                      \
        }                                                                                         \
    } while (0)

// traceKernel (the reference's order, render_manager.h:86-135) with the ray queue: one node visit
// per lane and iteration.
template <int STACK>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES))) void traceKernelQ(DevScene S, const pt_ray* rays, int64_t n, float tmin,
                                                      float tmax, pt_hit* hits, unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    Counters c{0, 0, 0, 0};
    int64_t ray = -1, poolBase = 0;
    uint32_t poolLeft = 0u;
    bool more = true;
    BinWalk w = {};
    float closest = 0.0f;
    int best = -1;
    for (;;) {
        bool took = false;
        PT_TRACE_REFILL(took);
        if (__ballot(ray >= 0) == 0) break;
        if (ray < 0) continue;
        if ((took && binStart<false>(S, rays[ray], tmin, tmax, w, closest, best, c)) ||
            binVisit<STACK, false>(S, my, tmin, w, closest, best, c)) {
            hits[ray] = binHit(S, best, closest, w.o, w.d);
            ray = -1;
        }
    }
    flushCounters(counters, c);
}

// traceKernelWide with the ray queue: per lane and iteration, the current primitive group's tests
// and one node (or instance entry) of the wide traversal.
template <int STACK, bool INST>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES))) void traceKernelWideQ(DevScene S, const pt_ray* rays, int64_t n, float tmin,
                                                          float tmax, pt_hit* hits, unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    const __amdgpu_buffer_rsrc_t nodeRsrc = rawRsrc(S.wnodes);
    Counters c{0, 0, 0, 0};
    int64_t ray = -1, poolBase = 0;
    uint32_t poolLeft = 0u;
    bool more = true;
    WideWalk w = {};
    WideBest b = {0.0f, 0.0f, -1, false};
    for (;;) {
        bool took = false;
        PT_TRACE_REFILL(took);
        if (__ballot(ray >= 0) == 0) break;
        if (ray < 0) continue;
        if (took) wideStartClosest<INST>(S, rays[ray], tmin, tmax, w, b, c);
        wideGroupClosest<INST>(S, w, b, c);
        if (wideStep<STACK, INST>(S, nodeRsrc, my, b.closest, w, c)) {
            if (PT_TRACE_DIAG_REDO && b.redo) c.spheres++;
            pt_hit h = wideHit<INST>(S, w, b, tmin, tmax);
            if (PT_TRACE_DIAG_VISITS) h.mat = (int)w.visits;
            hits[ray] = h;
            ray = -1;
        }
    }
    flushCounters(counters, c);
}

// pt_render_aov: traceKernelWideQ's walk (the same queue and steps) of the camera rays through the
// pixel centres of a film's rows, made from the pixel index instead of loaded, over [0.001, inf); the
// result is the pixel's three 16-byte guide rows {albedo, depth}{n, obj}{p, mat} (include/pt.h, pt_aov)
// instead of a pt_hit.  The camera waits in LDS and is read where a lane takes a pixel: held in SGPRs across
// the walk's loop its 18 words would not fit beside the walk's own (the trace kernels use all 102).
struct AovCam {
    float pos[3], ll[3], hor[3], ver[3];
    float invW, invH;
    int width, stripe_h, nparts, part;
};
constexpr int kAovCamWords = sizeof(AovCam) / 4;
template <int STACK, bool INST>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES))) void aovKernelWideQ(DevScene S, AovCam cam, int64_t n,
                                                          float4* out, unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    const __amdgpu_buffer_rsrc_t nodeRsrc = rawRsrc(S.wnodes);
    __shared__ uint32_t camWords[kAovCamWords];
    if (lane < kAovCamWords) camWords[lane] = reinterpret_cast<const uint32_t*>(&cam)[lane];
    __syncthreads();
    const volatile uint32_t* cw = camWords;   // (volatile: read at each use, not kept in registers across the loop)
    const auto camF = [&](int i) { return __uint_as_float(cw[i]); };
    const float tmin = 0.001f, tmax = __builtin_inff();
    Counters c{0, 0, 0, 0};
    int64_t ray = -1, poolBase = 0;
    uint32_t poolLeft = 0u;
    bool more = true;
    WideWalk w = {};
    WideBest b = {0.0f, 0.0f, -1, false};
    for (;;) {
        bool took = false;
        PT_TRACE_REFILL(took);
        if (__ballot(ray >= 0) == 0) break;
        if (ray < 0) continue;
        if (took) {
            const int width = (int)cw[14];
            const int lrow = (int)(ray / width), col = (int)(ray - (int64_t)lrow * width);
            const float u = ((float)col + 0.5f) * camF(12);
            const float v = ((float)globalRow(lrow, (int)cw[15], (int)cw[16], (int)cw[17]) + 0.5f) * camF(13);
            const float3 pos = f3(camF(0), camF(1), camF(2));
            const float3 d = sub(add(add(f3(camF(3), camF(4), camF(5)), scale(u, f3(camF(6), camF(7), camF(8)))),
                                     scale(v, f3(camF(9), camF(10), camF(11)))), pos);
            const pt_ray r = {{pos.x, pos.y, pos.z}, {d.x, d.y, d.z}};
            wideStartClosest<INST>(S, r, tmin, tmax, w, b, c);
        }
        wideGroupClosest<INST>(S, w, b, c);
        if (wideStep<STACK, INST>(S, nodeRsrc, my, b.closest, w, c)) {
            HitRec x;
            float t;
            float4 r0 = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
            float4 r1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), r2 = r1;
            if (wideHitRec<INST>(S, w, b, tmin, tmax, x, t)) {
                if (x.type == PT_LAMBERTIAN || x.type == PT_METAL) { r0.x = x.m0.x; r0.y = x.m0.y; r0.z = x.m0.z; }
                else if (x.type == PT_EMISSIVE) { r0.x = fminf(x.m0.x, 1.0f); r0.y = fminf(x.m0.y, 1.0f); r0.z = fminf(x.m0.z, 1.0f); }
                r0.w = t * sqrtf((w.wd.x * w.wd.x + w.wd.y * w.wd.y) + w.wd.z * w.wd.z);
                r1 = make_float4(x.n.x, x.n.y, x.n.z, __int_as_float(x.obj));
                r2 = make_float4(x.p.x, x.p.y, x.p.z, __int_as_float(x.mat));
            }
            float4* o = out + 3 * (size_t)ray;
            o[0] = r0; o[1] = r1; o[2] = r2;
            ray = -1;
        }
    }
    flushCounters(counters, c);
}

// ------------------------------------------------------------------------ occlusion (any hit)
// pt_trace_occluded: occ[i] = 1 exactly when the closest-hit query of ray i over [tmin, tmax_i]
// reports a hit (DESIGN.md "Occlusion queries").  The reference's traversal accepts a hit iff some
// primitive P passes (a) primHitT(P, o, d, tmin, tmax) >= 0 and (b) the scene has one primitive,
// or P's exact leaf box passes the slab test over [tmin, tmax] (refLeafBox): `closest` only
// shrinks once a hit exists, ancestor boxes contain the leaf box (monotonic slab arithmetic,
// traceRefStackless) and the wide planes never reject a box the exact test accepts (wideHits).
// So the walk keeps the interval fixed and stops at the first primitive that passes (a) and (b):
// the closest-hit kernels' walk up to their first accepted hit, hence never more work.
// rayTmax (optional): per-ray tmax, replacing the scalar.  A NaN entry is no upper bound (include/pt.h)
// and is replaced by +inf where it is read, so no later test sees it.  Left in place it is +inf to
// every `bound < x` comparison and NaN-ignoring min, with two exceptions: a signalling NaN (in IEEE
// mode v_min_f32 / v_min3_f32 return NaN for a signalling operand, and the wide node test's raw
// v_min3_f32, min3Raw, then rejects every box), and a node all of whose far planes are NaN (an
// instanced scene's ray with three zero or denormal direction components: min(NaN planes, NaN) is
// NaN where min(NaN planes, inf) is inf).
__device__ __forceinline__ float rayTmaxOf(const float* __restrict__ rayTmax, int64_t ray, float tmax) {
    if (!rayTmax) return tmax;
    const float t = rayTmax[ray];
    return t != t ? __builtin_inff() : t;
}

// pt_trace_occluded on the binary LBVH (PT_KERNEL_SIMPLE / PT_KERNEL_WAVEFRONT): traceKernelQ's walk
// (binStart / binVisit with ANY) with the interval fixed at the ray's tmax; a lane stops at the
// first accepted primitive and takes the next ray.
template <int STACK>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES))) void occludedKernelQ(
    DevScene S, const pt_ray* rays, int64_t n, float tmin, float tmax, const float* __restrict__ rayTmax, uint8_t* occ,
    unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    Counters c{0, 0, 0, 0};
    int64_t ray = -1, poolBase = 0;
    uint32_t poolLeft = 0u;
    bool more = true;
    BinWalk w = {};
    float tmaxR = 0.0f;
    int best = -1;
    for (;;) {
        bool took = false;
        PT_TRACE_REFILL(took);
        if (__ballot(ray >= 0) == 0) break;
        if (ray < 0) continue;
        if ((took && binStart<true>(S, rays[ray], tmin, rayTmaxOf(rayTmax, ray, tmax), w, tmaxR, best, c)) ||
            binVisit<STACK, true>(S, my, tmin, w, tmaxR, best, c)) {
            occ[ray] = best >= 0 ? 1 : 0;
            ray = -1;
        }
    }
    flushCounters(counters, c);
}

// pt_trace_occluded on the wide tree: traceKernelWideQ's walk (ray queue, wideStart, wideStep:
// node loads, node tests, nearest-first child order) with the interval fixed at the ray's tmax,
// one lane per ray; a lane stops at the first primitive that passes the contract's test and takes
// the next ray.  A far origin or a direction the MIX planes cannot take (wideFar, mixUnsafe) is
// answered by the reference-order query's flag, as in the closest-hit kernel (no work counted
// there either).  INST: the two-level walk; no leaf boxes, so the test is (a) alone in the
// instance's space.
template <int STACK, bool INST>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES))) void occludedKernelWideQ(
    DevScene S, const pt_ray* rays, int64_t n, float tmin, float tmax, const float* __restrict__ rayTmax, uint8_t* occ,
    unsigned long long* counters) {
    __shared__ uint32_t stk[STACK * kWave];
    const int lane = threadIdx.x;
    uint32_t* my = stk + lane;
    const __amdgpu_buffer_rsrc_t nodeRsrc = rawRsrc(S.wnodes);
    Counters c{0, 0, 0, 0};
    int64_t ray = -1, poolBase = 0;
    uint32_t poolLeft = 0u;
    bool more = true;
    WideWalk w = {};
    float tmaxI = 0.0f;
    for (;;) {
        bool took = false;
        PT_TRACE_REFILL(took);
        if (__ballot(ray >= 0) == 0) break;
        if (ray < 0) continue;
        bool hit = false, fin = false;
        if (took) {
            const float tmaxR = rayTmaxOf(rayTmax, ray, tmax);
            if (wideStart<INST>(S, rays[ray], tmin, tmaxR, w, tmaxI, c)) {   // the query in the reference's order: its flag
                float closest = tmaxR;
                hit = traceRefStackless(S, w.o, w.d, tmin, closest) >= 0;
                fin = true;
            }
        }
        while (w.tg && !hit) {
            const uint32_t k = w.tgBase + (uint32_t)__builtin_ctz(w.tg);
            w.tg &= w.tg - 1u;
            const float4* p = S.wprims + 3 * (size_t)k;
            const Prim q{p[0], p[1], p[2]};
            const bool sph = __float_as_uint(q.p2.w) != 0u;
            if (sph) c.spheres++;
            else c.tris++;
            hit = primHitT(q, sph, w.o, w.d, w.tminI, tmaxI) >= 0.0f &&
                  (INST || S.nprims <= 1 || refLeafBox(q, sph, w.o, w.inv, w.tminI, tmaxI).hit);
        }
        if (fin || hit || wideStep<STACK, INST>(S, nodeRsrc, my, tmaxI, w, c)) {
            occ[ray] = hit ? 1 : 0;
            ray = -1;
        }
    }
    flushCounters(counters, c);
}

// initRandom (main.cu:262-269): curand_init(seed, pixel, 0).  The subsequence skip is the
// GF(2) product of jump matrices J_k = M^(2^(67+k)) for the set bits of the pixel index.
// Loops are wave-uniform (k, j); column loads are uniform, hence scalar.
__global__ __launch_bounds__(256) void rngInitKernel(uint32_t* sd, uint32_t* s0, uint32_t* s1, uint32_t* s2,
                                                     uint32_t* s3, uint32_t* s4, const uint32_t* __restrict__ jm,
                                                     uint64_t seed, int width, int nrows, int sh, int nparts,
                                                     int part) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npix = (int64_t)width * nrows;
    if (idx >= npix) return;
    const int lrow = (int)(idx / width), col = (int)(idx % width);
    const uint64_t pixel = (uint64_t)globalRow(lrow, sh, nparts, part) * (uint64_t)width + (uint64_t)col;
    const uint32_t a = (uint32_t)seed ^ 0xaad26b49u, b = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * a, t1 = 2591861531u * b;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    const uint32_t d = 6615241u + t1 + t0;
    for (int k = 0; k < kJumpMats; k++) {
        if (!((pixel >> k) & 1u)) continue;
        const uint32_t* m = jm + (size_t)k * 160 * 5;
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (int j = 0; j < 160; j++) {
            const uint32_t bit = (v[j >> 5] >> (j & 31)) & 1u;
            const uint32_t mask = 0u - bit;
#pragma unroll
            for (int w = 0; w < 5; w++) r[w] ^= m[j * 5 + w] & mask;
        }
#pragma unroll
        for (int w = 0; w < 5; w++) v[w] = r[w];
    }
    sd[idx] = d; s0[idx] = v[0]; s1[idx] = v[1]; s2[idx] = v[2]; s3[idx] = v[3]; s4[idx] = v[4];
}

// --- LBVH (utils/bvh.h:17-130) -----------------------------------------------------------
__device__ __forceinline__ int deltaK(const unsigned long long* k, long long n, long long i, long long j) {   // morton_code.h:47-54
    if (i < 0 || i >= n || j < 0 || j >= n) return -1;
    return __clzll(k[i] ^ k[j]);
}

// generateLBVH (bvh.h:71-115) with the node reset separated from the linking (no race):
// writes child refs of internal node i and the parent link of both children.
__global__ void karrasKernel(const unsigned long long* __restrict__ keys, int n, float4* nodes, int* iparent,
                             int* lparent, const uint32_t* __restrict__ leafSphere, int2* irange) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    // determineRange (bvh.h:17-40)
    const int ld = deltaK(keys, n, i, i - 1), rd = deltaK(keys, n, i, i + 1);
    const int dir = (rd - ld > 0) - (rd - ld < 0);
    const int dmin = min(ld, rd);
    long long maxStride = 2;
    while (deltaK(keys, n, i, i + maxStride * dir) > dmin) maxStride *= 2;
    long long l = 0;
    for (long long s = maxStride >> 1; s >= 1; s >>= 1)
        if (deltaK(keys, n, i, i + (l + s) * dir) > dmin) l += s;
    int first = i, last = (int)(i + l * dir);
    if (dir < 0) { int t = first; first = last; last = t; }
    // findSplit (bvh.h:42-69)
    const unsigned long long fc = keys[first], lc = keys[last];
    int split;
    if (first == last) {
        split = (first + last) >> 1;
    } else {
        const int common = __clzll(fc ^ lc);
        split = first;
        int step = last - first;
        do {
            step = (step + 1) >> 1;
            const int ns = split + step;
            if (ns < last && __clzll(fc ^ keys[ns]) > common) split = ns;
        } while (step > 1);
    }
    uint32_t a, b;
    if (split == first) { a = kLeafBit | (leafSphere[split] ? kSphereBit : 0u) | (uint32_t)split; lparent[split] = i; }
    else { a = (uint32_t)split; iparent[split] = i; }
    if (split + 1 == last) { b = kLeafBit | (leafSphere[split + 1] ? kSphereBit : 0u) | (uint32_t)(split + 1); lparent[split + 1] = i; }
    else { b = (uint32_t)(split + 1); iparent[split + 1] = i; }
    nodes[4 * (size_t)i + 3] = make_float4(__uint_as_float(a), __uint_as_float(b), 0.0f, 0.0f);
    irange[i] = make_int2(first, last);   // leaf range (the device wide build's ranks)
}

// growBBox (bvh.h:117-130) as a correct bottom-up refit: every leaf writes its box into its
// parent's slot, then climbs; the second thread to reach a node unions the node's two child boxes
// into the grandparent's slot.  Tight boxes.
//
// No agent-scope synchronisation (its acq_rel fence is an L2 writeback + invalidate on this
// multi-L2 chip: the all-global version spent 3.7 ms of a 5-ms C5 build in them).  Phase 1: a
// workgroup owns the 256 leaves [base, base + 256); a node whose leaf range lies inside them
// (Karras: node i is an end of its own range, so i is in the block too) is completed in LDS with
// workgroup-scope counters.  A thread reaching a node whose range crosses a block boundary
// stores its box in that node's slot and records the arrival (events).  Phase 2: one workgroup
// replays the arrivals with workgroup-scope counters in global memory -- the crossing nodes are
// the top of the tree, about 1/16 of the nodes.
constexpr int kRefitBlock = 256, kRefitTop = 1024;
__global__ __launch_bounds__(kRefitBlock) void refitKernel(float4* nodes, const int* __restrict__ iparent,
                                                           const int* __restrict__ lparent, const int2* __restrict__ irange,
                                                           const float* __restrict__ leafBoxes, unsigned int* events, int n) {
    __shared__ float sbox[kRefitBlock][2][6];   // child boxes of the block's internal nodes
    __shared__ unsigned int scnt[kRefitBlock];
    const int base = blockIdx.x * kRefitBlock, end = min(base + kRefitBlock, n);
    scnt[threadIdx.x] = 0u;
    __syncthreads();
    const int k = base + (int)threadIdx.x;
    if (k >= n) return;
    float b[6];
    for (int i = 0; i < 6; i++) b[i] = leafBoxes[6 * (size_t)k + i];
    int p = lparent[k];
    int self = k;
    bool leaf = true;
    for (int guard = 0; p >= 0 && guard < 130; guard++) {
        const float4 refs = nodes[4 * (size_t)p + 3];
        const uint32_t lref = __float_as_uint(refs.x);
        const bool isLeft = leaf ? ((lref & kLeafBit) && (int)(lref & kPrimMask) == self)
                                 : (!(lref & kLeafBit) && (int)lref == self);
        float* f = reinterpret_cast<float*>(nodes + 4 * (size_t)p);
        for (int i = 0; i < 6; i++) f[nodeBoxIdx(isLeft ? 0 : 1, i % 3, i / 3)] = b[i];
        const int2 range = irange[p];
        if (range.x < base || range.y >= end) {   // crossing: phase 2 finishes it
            events[1 + atomicAdd(events, 1u)] = (unsigned)p;
            return;
        }
        for (int i = 0; i < 6; i++) sbox[p - base][isLeft ? 0 : 1][i] = b[i];
        const unsigned int prev = __hip_atomic_fetch_add(&scnt[p - base], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (prev == 0) return;   // sibling not done yet: it will carry on
        for (int i = 0; i < 3; i++) {   // utils::unionBox (aabb.h:55-65)
            b[i] = fminf(sbox[p - base][0][i], sbox[p - base][1][i]);
            b[3 + i] = fmaxf(sbox[p - base][0][3 + i], sbox[p - base][1][3 + i]);
        }
        self = p;
        leaf = false;
        p = iparent[p];
    }
}

__global__ __launch_bounds__(kRefitTop) void refitTopKernel(float4* nodes, const int* __restrict__ iparent,
                                                            const unsigned int* __restrict__ events, unsigned int* arrivals) {
    const unsigned int count = events[0];
    for (unsigned int e = threadIdx.x; e < count; e += kRefitTop) {
        int p = (int)events[1 + e];
        for (int guard = 0; p >= 0 && guard < 130; guard++) {
            const unsigned int prev = __hip_atomic_fetch_add(arrivals + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (prev == 0) break;   // the other child is not done yet
            const float* f = reinterpret_cast<const float*>(nodes + 4 * (size_t)p);
            float b[6];
            for (int i = 0; i < 3; i++) {   // utils::unionBox (aabb.h:55-65)
                b[i] = fminf(f[nodeBoxIdx(0, i, 0)], f[nodeBoxIdx(1, i, 0)]);
                b[3 + i] = fmaxf(f[nodeBoxIdx(0, i, 1)], f[nodeBoxIdx(1, i, 1)]);
            }
            const int q = iparent[p];
            if (q < 0) break;
            const uint32_t lref = __float_as_uint(nodes[4 * (size_t)q + 3].x);
            const bool isLeft = !(lref & kLeafBit) && (int)lref == p;
            float* g = reinterpret_cast<float*>(nodes + 4 * (size_t)q);
            for (int i = 0; i < 6; i++) g[nodeBoxIdx(isLeft ? 0 : 1, i % 3, i / 3)] = b[i];
            p = q;
        }
    }
}

// --- Morton keys and leaf records on the device (morton_code.h:19-75, cuda_object.h:21-42) ----
// Each expression restates the host computation (pt_host.cpp mortonKeys / the leaf loop of
// pt_scene_build_bvh) in the same operation order, so keys, boxes and normals are bit-identical.

// Object box (cuda_object.h:21-42): sphere c -/+ |r|; triangle utils::unionPoints by comparisons.
__device__ __forceinline__ void objBoxDev(const pt_object& o, float mn[3], float mx[3]) {
    if (o.type == PT_SPHERE) {
        const float r = fabsf(o.v[3]);
        for (int a = 0; a < 3; a++) { mn[a] = o.v[a] - r; mx[a] = o.v[a] + r; }
        return;
    }
    for (int a = 0; a < 3; a++) {
        mn[a] = o.v[a];
        mx[a] = o.v[a];
    }
    for (int k = 1; k < 3; k++)
        for (int a = 0; a < 3; a++) {
            const float p = o.v[3 * k + a];
            if (mn[a] > p) mn[a] = p;
            if (mx[a] < p) mx[a] = p;
        }
}

// Scene box for the Morton quantisation (main.cu:122 + aabb::unionBoxInPlace, aabb.h:36-44):
// min/max are exact and order-independent, so one workgroup reduces all boxes.  The reference
// seeds the box with aabb() = the zero box (includeOrigin), or the first object's box.  Two
// launches: per-block boxes over a grid-stride range (partial[6 * block]), then their union.
constexpr int kBoxBlocks = 512;
__global__ __launch_bounds__(1024) void sceneBoxKernel(const pt_object* __restrict__ objs, int64_t n,
                                                       int includeOrigin, float* box6, float* partial) {
    __shared__ float red[6][1024];
    float b[6];
    const bool final = partial == nullptr;   // the second launch: union of the per-block boxes in box6 + 6
    if (final || includeOrigin) {
        for (int a = 0; a < 6; a++) b[a] = final ? (a < 3 ? INFINITY : -INFINITY) : 0.0f;
        if (final && includeOrigin)
            for (int a = 0; a < 6; a++) b[a] = 0.0f;
    } else {
        objBoxDev(objs[0], b, b + 3);
    }
    if (final) {
        const float* pb = box6 + 6;
        if (!includeOrigin && threadIdx.x == 0) objBoxDev(objs[0], b, b + 3);
        for (int i = threadIdx.x; i < kBoxBlocks; i += blockDim.x)
            for (int a = 0; a < 3; a++) {
                b[a] = fminf(b[a], pb[6 * i + a]);
                b[3 + a] = fmaxf(b[3 + a], pb[6 * i + 3 + a]);
            }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            float mn[3], mx[3];
            objBoxDev(objs[i], mn, mx);
            for (int a = 0; a < 3; a++) {
                b[a] = fminf(b[a], mn[a]);
                b[3 + a] = fmaxf(b[3 + a], mx[a]);
            }
        }
    }
    for (int a = 0; a < 6; a++) red[a][threadIdx.x] = b[a];
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 3; a++) {
                red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + w]);
                red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) (final ? box6 : partial + 6 * blockIdx.x)[threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ uint32_t expandBitsDev(uint32_t v) {   // morton_code.h:19-27
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

// mortonCode3D (morton_code.h:29-45): centre normalised into the scene box (an axis whose
// range is <= 1e-7 maps to 0), x1024, clamped to [0, 1023], truncated, interleaved.
__global__ __launch_bounds__(256) void mortonKernel(const pt_object* __restrict__ objs, int64_t n,
                                                    const float* __restrict__ box6, uint32_t* codes, uint32_t* ids) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float mn[3], mx[3];
    objBoxDev(objs[i], mn, mx);
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float smn = box6[a], range = box6[3 + a] - box6[a];
        const float c = (mn[a] + mx[a]) * 0.5f;
        float x = 0.0f;
        if ((double)range > 1e-7) x = (c - smn) / range;
        q[a] = (uint32_t)fminf(fmaxf(x * 1024.0f, 0.0f), 1023.0f);
    }
    codes[i] = (expandBitsDev(q[0]) << 2) + (expandBitsDev(q[1]) << 1) + expandBitsDev(q[2]);
    ids[i] = (uint32_t)i;
}

// Leaf k of the sorted order: the 64-bit key (code << 32 | objID, the MORTON64 union of
// morton_code.h), the primitive record, the triangle normal (triangle.h:17-19:
// normalize(cross(v1 - v0, v2 - v0))), the exact leaf box and the sphere flag.
__global__ __launch_bounds__(256) void leafGatherKernel(const pt_object* __restrict__ objs,
                                                        const uint32_t* __restrict__ codes,
                                                        const uint32_t* __restrict__ ids, int64_t n,
                                                        unsigned long long* keys, float4* prims, float4* shade,
                                                        float* boxes, uint32_t* sphereFlag,
                                                        const float4* __restrict__ mats) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t id = ids[k];
    const pt_object o = objs[id];
    keys[k] = ((unsigned long long)codes[k] << 32) | id;
    float mn[3], mx[3];
    objBoxDev(o, mn, mx);
    for (int a = 0; a < 3; a++) { boxes[6 * k + a] = mn[a]; boxes[6 * k + 3 + a] = mx[a]; }
    if (o.type == PT_SPHERE) {
        prims[3 * k] = make_float4(o.v[0], o.v[1], o.v[2], __uint_as_float((uint32_t)o.mat));
        prims[3 * k + 1] = make_float4(o.v[3], 0.0f, 0.0f, __uint_as_float(id));
        prims[3 * k + 2] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(1u));
        shade[3 * k] = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
        sphereFlag[k] = 1u;
    } else {
        const float3 v0 = f3(o.v[0], o.v[1], o.v[2]), v1 = f3(o.v[3], o.v[4], o.v[5]), v2 = f3(o.v[6], o.v[7], o.v[8]);
        const float3 nn = normalize3(cross3(sub(v1, v0), sub(v2, v0)));
        prims[3 * k] = make_float4(v0.x, v0.y, v0.z, __uint_as_float((uint32_t)o.mat));
        prims[3 * k + 1] = make_float4(v1.x, v1.y, v1.z, __uint_as_float(id));
        prims[3 * k + 2] = make_float4(v2.x, v2.y, v2.z, 0.0f);
        shade[3 * k] = make_float4(nn.x, nn.y, nn.z, 0.0f);
        sphereFlag[k] = 0u;
    }
    // the object's material inline: {albedo, fuzz}, {ir, type | sphere << 16, mat, obj}
    const float4 m0 = mats[2 * o.mat], m1 = mats[2 * o.mat + 1];
    shade[3 * k + 1] = m0;
    shade[3 * k + 2] = make_float4(m1.x, __uint_as_float(__float_as_uint(m1.y) | (o.type == PT_SPHERE ? 0x10000u : 0u)),
                                   __uint_as_float((uint32_t)o.mat), __uint_as_float(id));
}

// The sampled lights of PT_RENDER_NEE (pt.h): the emissive triangles, compacted in object order.
// lightFlagKernel marks them, an exclusive scan (pt_prims.hpp) gives each its slot, lightListKernel
// writes the records {v0}{e1 = v1 - v0}{e2 = v2 - v0}{E} and the count.
__global__ __launch_bounds__(256) void lightFlagKernel(const pt_object* __restrict__ objs, int64_t n,
                                                       const float4* __restrict__ mats, uint32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool light = objs[i].type == PT_TRIANGLE && __float_as_uint(mats[2 * objs[i].mat + 1].y) == (uint32_t)PT_EMISSIVE;
    flag[i] = light ? 1u : 0u;
}
__global__ __launch_bounds__(256) void lightListKernel(const pt_object* __restrict__ objs, int64_t n,
                                                       const float4* __restrict__ mats,
                                                       const uint32_t* __restrict__ flag,
                                                       const uint32_t* __restrict__ slot, uint32_t cap, float4* lights,
                                                       uint32_t* count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *count = slot[i] + flag[i];
    if (!flag[i] || slot[i] >= cap) return;   // (cap: the records the host reserved; it counted the same objects)
    const pt_object o = objs[i];
    const float3 v0 = f3(o.v[0], o.v[1], o.v[2]), v1 = f3(o.v[3], o.v[4], o.v[5]), v2 = f3(o.v[6], o.v[7], o.v[8]);
    const float3 e1 = sub(v1, v0), e2 = sub(v2, v0);
    const float4 m0 = mats[2 * o.mat];
    float4* L = lights + 4 * (size_t)slot[i];
    L[0] = make_float4(v0.x, v0.y, v0.z, 0.0f);
    L[1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
    L[2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
    L[3] = make_float4(m0.x, m0.y, m0.z, 0.0f);
}

// Depth of the internal hierarchy (root = 1) = the most internal ancestors of any leaf.
__global__ __launch_bounds__(256) void depthKernel(const int* __restrict__ iparent, const int* __restrict__ lparent,
                                                   int n, int* depth) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int d = 0;
    for (int p = lparent[k]; p >= 0 && d <= n; p = iparent[p]) d++;
    atomicMax(depth, d);
}

// ------------------------------------------------------------------------ host helpers
// GF(2) 160x160 jump matrices for XORWOW's xorshift part (product-side implementation).
struct Mat160 { uint32_t c[160][5]; };

void apply160(const Mat160& m, const uint32_t in[5], uint32_t out[5]) {
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int j = 0; j < 160; j++) {
        const uint32_t mask = 0u - ((in[j / 32] >> (j % 32)) & 1u);
        for (int w = 0; w < 5; w++) r[w] ^= m.c[j][w] & mask;
    }
    std::memcpy(out, r, sizeof(r));
}

const std::vector<uint32_t>& jumpMatrices() {
    static const std::vector<uint32_t> tables = [] {
        Mat160 m;
        for (int j = 0; j < 160; j++) {   // image of basis vector e_j under one xorshift step
            uint32_t v[5] = {0, 0, 0, 0, 0};
            v[j / 32] = 1u << (j % 32);
            const uint32_t t = v[0] ^ (v[0] >> 2);
            const uint32_t nv[5] = {v[1], v[2], v[3], v[4], (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))};
            std::memcpy(m.c[j], nv, sizeof(nv));
        }
        auto sq = [](const Mat160& a) {
            Mat160 r;
            for (int j = 0; j < 160; j++) apply160(a, a.c[j], r.c[j]);
            return r;
        };
        for (int i = 0; i < 67; i++) m = sq(m);
        std::vector<uint32_t> out((size_t)kJumpMats * 160 * 5);
        for (int k = 0; k < kJumpMats; k++) {
            std::memcpy(&out[(size_t)k * 800], m.c, sizeof(m.c));
            m = sq(m);
        }
        return out;
    }();
    return tables;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;   // bytes allocated
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <class T> T* as() const { return static_cast<T*>(p); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

int devAlloc(DevBuf& b, size_t bytes) {
    b.reset();
    if (bytes == 0) bytes = 16;
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return PT_OK;
}
// Keeps the buffer when it is large enough (no hipFree / hipMalloc, which synchronise the device:
// a per-frame BVH rebuild reuses every buffer of the previous build).
int devReserve(DevBuf& b, size_t bytes) {
    if (b.p && b.cap >= std::max<size_t>(bytes, 16)) return PT_OK;
    return devAlloc(b, bytes);
}

// (envInt, envCount: host/pt_render_plan.hpp)

// One stable radix sort of (key, id) pairs by the keys' low `bits` bits, ascending: the size query,
// `temp` grown to it (kept by its owner between calls), the sort.
int sortPairs(DevBuf& temp, const uint32_t* keys, uint32_t* keys2, const uint32_t* ids, uint32_t* ids2, size_t n, int bits,
              hipStream_t st) {
    size_t bytes = 0;
    HIP_TRY(pt::radixSortPairs(nullptr, &bytes, keys, keys2, ids, ids2, n, bits, st));
    if (int rc = devReserve(temp, bytes)) return rc;
    HIP_TRY(pt::radixSortPairs(temp.p, &bytes, keys, keys2, ids, ids2, n, bits, st));
    return PT_OK;
}

// Events of a synchronous device step; on an early return (ok still false) the stream's queued
// work is waited for before the caller can free or reuse what it reads.
struct StreamGuard {
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = false;
    explicit StreamGuard(hipStream_t s) : st(s) {}
    ~StreamGuard() {
        if (!ok) (void)hipStreamSynchronize(st);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// A pair of events kept with their owner (a per-frame build times itself without creating any).
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};
// On an early return (ok still false) waits for the stream's queued work, as StreamGuard does.
struct StreamWait {
    hipStream_t st;
    bool ok = false;
    explicit StreamWait(hipStream_t s) : st(s) {}
    ~StreamWait() {
        if (!ok) (void)hipStreamSynchronize(st);
    }
};

// (stackFor: host/pt_render_plan.hpp)
// The instanced scene's host tree build, mixLimit and wideStackFor: host/pt_instancing.cpp
using pt::InstEntry;
using pt::instanceInverse;
using pt::mixLimit;
using pt::wideStackFor;

}  // namespace

// ================================================================== opaque objects
struct pt_scene {
    int device = 0;
    int64_t nobj = 0, nmat = 0;
    bool hasSpheres = false;                // any sphere ever in the scene (sticky across updates)
    std::vector<pt_object> objs;            // host copy (PT_BVH_HOST_KEYS path)
    DevBuf dobjs;                           // the objects on the device (BVH build input)
    DevBuf mats, nodes, prims, shade, counters;
    DevBuf keys, iparent, lparent, leafBoxes;   // sorted 64-bit Morton keys, parent links, leaf boxes
    // build scratch, kept between builds: codes / ids (unsorted, sorted), scene box, sphere
    // flags, refit arrival counters, depth, sort temporary
    DevBuf codes, ids, codes2, ids2, box6, sph, arr, dep, sortTemp;
    DevBuf irange;                          // leaf range [first, last] per internal node
    DevBuf refitEvents;                     // refit phase 2 input: count, then crossing-node arrivals
    DevBuf wide, wprims, wshade, rankOf;    // compressed 8-wide tree, its primitive and shading records, leaf ranks (PT_KERNEL_WIDE)
    DevBuf wbox;                            // exact primitive boxes in rank order (DevScene::wbox)
    DevBuf wtris;                           // wprims in edge form (pt::edgeTriRecords): what the render kernels' LEAF step reads
    bool haveWtris = false;                 // wtris matches wprims (built with the wide tree of a triangle-only scene)
    std::unique_ptr<pt::WideDevBuilder> wideDev;   // device build scratch (PT_BVH_WIDE_DEVICE), kept between builds
    bool wideReady = false;                 // the wide tree matches the current LBVH build
    bool updated = false;                   // pt_scene_update_objects was called: a dynamic scene
    int wideSource = 0;                     // 1: host binned SAH, 2: device SAH / PLOC, 3: instanced (full build), 4: instanced (top level only)
    int wideDepth = 0;
    int64_t wideNodes = 0;                  // node slots
    double wideBuildMs = 0.0;               // host build + upload, wall time
    int depth = 0;
    bool built = false;
    size_t deviceBytes = 0;
    double buildMs = 0.0;                   // last pt_scene_build_bvh, device time (HIP events)
    float sceneCE[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // tight scene box: centre, largest extent (DevScene)
    float skyH[3] = {1.0f, 1.0f, 1.0f}, skyZ[3] = {0.5f, 0.7f, 1.0f};   // pt_scene_set_sky (default: main.cu:34-36)
    bool hasEmissive = false;               // any PT_EMISSIVE material
    bool lambertOnly = true;                // no PT_METAL or PT_DIELECTRIC material: only the unit-sphere loop draws on a path
    // PT_RENDER_NEE: the sampled lights (emissive triangles) of the last build, listed on the device
    // (lightFlagKernel, a scan, lightListKernel); the buffers are kept between builds
    std::vector<uint8_t> matEmissive;       // per material: its type is PT_EMISSIVE
    DevBuf lights, lightFlag, lightSlot, lightScan, lightCount;
    int64_t nLights = 0;
    float mixLim = -1.0f;                          // DevScene::mixLim (-1: every ray takes the reference order)
    // instanced scenes (pt_scene_create_instanced): meshes = object ranges of `objs`, instances
    bool instanced = false;
    std::vector<int64_t> meshFirst, meshCount;
    std::vector<pt_instance> inst;
    DevBuf winst;                           // per instance: world-to-object rows, {objBase, identity}
    size_t instPrimBytes = 0, instShadeBytes = 0, instWinstBytes = 0;   // wprims, wshade, winst of the full build (pt_scene_download_wide)
    int gBits = 0;                          // hit key = instance << gBits | shading index
    // Instance updates (pt_scene_update_instances).  A full build of a dynamic scene lays the node
    // array out for them -- the top level's region reserved at its upper bound, the mesh trees
    // behind it, quantised for twice the current reach -- and keeps what the later builds need:
    // they redo only the matrix-dependent work (rebuildInstancedTop).
    bool instDynamic = false;               // instances were updated, or a build was given PT_BVH_WIDE_DEVICE
    bool instPrepared = false;              // the members below match the node array
    std::vector<double> instReach;          // per mesh: the reach its tree's planes were quantised for
    std::vector<InstEntry> instEntries;     // the top level's entries, instances in order
    std::vector<uint32_t> instMeshRoot;     // per mesh: its root's slot in the node array
    uint32_t instTopCap = 0;                // node slots reserved for the top level
    int instMaxDepthB = 0;                  // deepest mesh tree
    DevBuf instM, instDesc, instSub, instOut;   // matrices, pt::InstBoxDesc, sub-root boxes; {instance boxes, entry boxes}
    // the device top-level build's inputs (entry records {.., entry}, identity ranks, instEntries,
    // instMeshRoot), its leaf-order entry records and the record kernel's error word
    DevBuf instPrims, instRank, instEntriesDev, instMeshRootDev, instWprims, instErr;
    EventPair instEvents;                   // the later builds' timing events, created once
    std::vector<float> instHostM;           // their staging buffers, kept between builds
    // Sampled lights of an instanced scene (PT_BVH_LIGHTS; pt.h states the rule): one world-space record
    // per (instance, emissive triangle of its mesh) in `lights`, written by pt::instanceLights on every
    // build that has the bit.  The tables depend on the meshes only and are made by the full build: the
    // emissive triangles' object indices mesh by mesh (instLightObj), per instance where its mesh's run
    // starts there (instLightSrc) and its first record (instLightFirst, n + 1 entries), and in
    // `lightSlot` each shading record's rank among its mesh's lights (the MIS kernels' lookup).
    bool instLights = false;                // the last build had PT_BVH_LIGHTS
    bool instLightsPrepared = false;        // the tables and the record buffer match the meshes
    int64_t instLightTotal = 0;             // records: fixed under pt_scene_update_instances
    DevBuf instLightFirst, instLightSrc, instLightObj;
    std::vector<double> instHostBox;
};

struct pt_film {
    int device = 0;
    int width = 0, height = 0, stripe_h = 1, nparts = 1, part = 0;
    int nrows = 0;
    int64_t npix = 0;
    uint64_t seed = 0;
    DevBuf state;   // 6 x npix uint32 (SoA)
    DevBuf jumps;   // XORWOW jump matrices (for pt_film_reset)
    DevBuf tileCost, tileOrder;   // measured per-tile cost of the last launch; LPT launch order
    DevBuf tileXY, tileXYId;      // sample mode: tileOrder decoded (tileXYKernel), and the identity order decoded
    bool haveXYId = false;
    DevBuf tileKeys, tileKeys2, tileIds, sortTemp;   // the order's radix sort on the device
    bool haveOrder = false;
    int framesSinceCost = 0;      // sample mode: frames rendered since the tile costs were last measured
    DevBuf pixAcc, taskCounter;   // sample mode: per-pixel {x, y, z, rays} accumulators; task counter
    // compat mode, wide kernel: rays per pixel of the last launch, and the next launch's critical
    // pixels (the longest chains: their ids sorted by descending rays, and a flag per pixel)
    DevBuf pixRays, pixKeys, pixKeys2, pixIds, pixSorted, critFlag, critTemp;
    int critK = 0;                // critical pixels selected for the next compat launch (0: none yet)
    DevBuf stackSpill;            // sample mode on deep trees: traversal stack entries beyond LDS
    DevBuf sums;                  // compat mode: raw per-pixel sample sums of the frame (resolve input)
    DevBuf accum;                 // progressive rendering: fp32 RGB running sums of every accumulated frame
    DevBuf staging;               // device copy of a host output frame
    DevBuf aovStaging;            // pt_render_aov: device copy of a host output
    DevBuf dnA, dnB;              // pt_film_denoise: the passes' two scratch images, allocated at first use and kept
    DevBuf dnRgb, dnAov;          // pt_film_denoise with host pointers: device copies of the image (in, then out) and the guides
    // pt_film_temporal: the two history images (48 B per pixel; a call gathers from tpHist[tpCur] and writes
    // the other), allocated at first use and kept; the camera of the frame in tpHist[tpCur]; whether there
    // is one (cleared by pt_film_temporal_reset); with host pointers, device copies of rgb / out, aov, out_len
    DevBuf tpHist[2];
    DevBuf tpRgb, tpAov, tpLen;
    int tpCur = 0;
    bool tpHave = false;
    pt_camera tpCam = {};
    int64_t accumSamples = 0;     // samples per pixel in `accum`
    int cus = 0;                  // compute units of the device (persistent grid size)
    // The last render's work counters (rays, visits, tests, paths, error word), filled by its
    // kernels, and the events around its kernels: read by pt_film_stats (or by pt_render_ex when
    // it is given a pt_stats), so a render with stats == NULL never waits for the device.
    DevBuf counters;
    unsigned long long* hostCounters = nullptr;   // pinned: the counters copied back in stream order
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;   // kernels start / end, counters copied
    bool rendered = false;
    bool lastWide = false;
    ~pt_film() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (hostCounters) (void)hipHostFree(hostCounters);
    }
};

namespace {
// Build the compressed 8-wide tree on the host from the device's leaf-order primitive records
// and exact leaf boxes (host/pt_wide8.cpp) and upload it.
int buildWide(pt_scene* s) {
    const int64_t n = s->nobj;
    std::vector<uint32_t> prims((size_t)n * pt::kW8PrimDwords), shade((size_t)n * 12);
    std::vector<float> boxes((size_t)n * 6);
    HIP_TRY(hipMemcpy(prims.data(), s->prims.p, prims.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(shade.data(), s->shade.p, shade.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(boxes.data(), s->leafBoxes.p, boxes.size() * 4, hipMemcpyDeviceToHost));
    // the reference's leaf order over the binary LBVH (child refs are dwords 12, 13 of a node)
    std::vector<uint32_t> refs((size_t)std::max<int64_t>(1, n - 1) * 16);
    if (n > 1) HIP_TRY(hipMemcpy(refs.data(), s->nodes.p, (size_t)(n - 1) * 64, hipMemcpyDeviceToHost));
    const std::vector<uint32_t> rank = pt::referenceRanks(refs.data() + 12, refs.data() + 13, 16, n);
    std::vector<uint32_t> wshade(shade.size());
    for (int64_t k = 0; k < n; k++) std::memcpy(&wshade[(size_t)rank[k] * 12], &shade[(size_t)k * 12], 48);
    std::vector<float> wbox((size_t)n * pt::kW8BoxFloats);
    for (int64_t k = 0; k < n; k++)
        pt::exactTriBox(reinterpret_cast<const float*>(&prims[(size_t)k * pt::kW8PrimDwords]), &wbox[(size_t)rank[k] * pt::kW8BoxFloats]);
    pt::Wide8 w;
    std::string err;
    if (!pt::buildWide8(prims.data(), boxes.data(), rank.data(), n, w, err)) return fail(PT_ERR_STATE, err);
    int rc;
    s->haveWtris = !s->hasSpheres;
    if (s->haveWtris) {
        std::vector<uint32_t> wtris(w.prims.size());
        pt::edgeTriRecords(w.prims.data(), n, wtris.data());
        if ((rc = devReserve(s->wtris, wtris.size() * 4))) return rc;
        HIP_TRY(hipMemcpy(s->wtris.p, wtris.data(), wtris.size() * 4, hipMemcpyHostToDevice));
    }
    if ((rc = devReserve(s->wide, w.nodes.size() * 4)) || (rc = devReserve(s->wprims, w.prims.size() * 4)) ||
        (rc = devReserve(s->wshade, wshade.size() * 4)) || (rc = devReserve(s->rankOf, rank.size() * 4)) ||
        (rc = devReserve(s->wbox, wbox.size() * 4)))
        return rc;
    HIP_TRY(hipMemcpy(s->wbox.p, wbox.data(), wbox.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->wide.p, w.nodes.data(), w.nodes.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->wprims.p, w.prims.data(), w.prims.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->wshade.p, wshade.data(), wshade.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->rankOf.p, rank.data(), rank.size() * 4, hipMemcpyHostToDevice));
    s->wideDepth = w.depth;
    s->wideNodes = (int64_t)(w.nodes.size() / pt::kW8NodeDwords);
    s->wideSource = 1;
    return PT_OK;
}

// The same records built on the device from the LBVH build's leaf records (csrc/pt_wide_build.hip),
// enqueued on `st` (it synchronises with the stream once per clustering pass and wide level).
int buildWideDevice(pt_scene* s, hipStream_t st) {
    const int64_t n = s->nobj;
    int rc;
    if ((rc = devReserve(s->wide, (size_t)pt::wideDevNodeSlots(n) * pt::kW8NodeDwords * 4)) ||
        (rc = devReserve(s->wprims, (size_t)n * pt::kW8PrimDwords * 4)) || (rc = devReserve(s->wshade, (size_t)n * 48)) ||
        (rc = devReserve(s->rankOf, (size_t)n * 4)) || (rc = devReserve(s->wbox, (size_t)n * pt::kW8BoxFloats * 4)))
        return rc;
    s->haveWtris = !s->hasSpheres;
    if (s->haveWtris && (rc = devReserve(s->wtris, (size_t)n * pt::kW8PrimDwords * 4))) return rc;
    if (!s->wideDev) s->wideDev.reset(new pt::WideDevBuilder);
    pt::WideDevIn in{s->prims.as<float4>(), s->shade.as<float4>(), s->leafBoxes.as<float>(), s->nodes.as<float4>(),
                     s->iparent.as<int>(), s->lparent.as<int>(), s->irange.as<int2>(), n};
    pt::WideDevOut out{s->wide.as<uint32_t>(), s->wprims.as<uint32_t>(), s->wshade.as<float4>(), s->wbox.as<float4>(),
                       s->rankOf.as<uint32_t>(), s->haveWtris ? s->wtris.as<uint32_t>() : nullptr};
    std::string err;
    const hipError_t e = s->wideDev->build(in, out, st, err);
    if (e != hipSuccess) return fail(err.empty() ? PT_ERR_HIP : PT_ERR_STATE, err.empty() ? hipGetErrorString(e) : err);
    s->wideDepth = out.depth;
    s->wideNodes = out.slots;
    s->wideSource = 2;
    return PT_OK;
}

// Instanced scenes: the two-level tree is built on the host (host/pt_instancing.cpp); this is its
// device half.  What both builds read of the scene (the full build adds the materials and knobs):
pt::InstancedIn instancedIn(const pt_scene* s) {
    pt::InstancedIn in{};
    in.objs = s->objs.data();
    in.meshFirst = s->meshFirst.data();
    in.meshCount = s->meshCount.data();
    in.nMeshes = (int)s->meshFirst.size();
    in.inst = s->inst.data();
    in.nInst = (int64_t)s->inst.size();
    in.nmat = s->nmat;
    in.dynamic = s->instDynamic;
    in.farExt = kInstFarExt;
    return in;
}

// PT_BVH_LIGHTS, the full build's part: the per-mesh tables (host: a pass over the objects) and every
// buffer the light list needs, so that the later builds allocate nothing.
int prepareInstanceLights(pt_scene* s) {
    s->instLightsPrepared = false;
    const size_t nm = s->meshFirst.size(), ni = s->inst.size();
    std::vector<uint32_t> obj, rank, meshSrc(nm), meshN(nm), first(ni + 1), src(std::max<size_t>(1, ni));
    for (size_t m = 0; m < nm; m++) {
        meshSrc[m] = (uint32_t)obj.size();
        for (int64_t k = 0; k < s->meshCount[m]; k++) {
            const pt_object& o = s->objs[(size_t)(s->meshFirst[m] + k)];
            const bool light = s->hasEmissive && o.type == PT_TRIANGLE && s->matEmissive[(size_t)o.mat];
            rank.push_back(light ? (uint32_t)obj.size() - meshSrc[m] : 0u);   // (shading index order: mesh by mesh)
            if (light) obj.push_back((uint32_t)(s->meshFirst[m] + k));
        }
        meshN[m] = (uint32_t)obj.size() - meshSrc[m];
    }
    int64_t total = 0;
    for (size_t i = 0; i < ni; i++) {
        first[i] = (uint32_t)total;
        src[i] = meshSrc[(size_t)s->inst[i].mesh];
        total += meshN[(size_t)s->inst[i].mesh];
        if (total > (int64_t)1 << 26) return fail(PT_ERR_INVALID, "pt_scene_build_bvh: PT_BVH_LIGHTS: more than 2^26 light records");
    }
    first[ni] = (uint32_t)total;
    s->instLightTotal = total;
    if (total > 0) {
        struct Upload { DevBuf* buf; const void* src; size_t bytes; };
        const Upload up[] = {{&s->instLightFirst, first.data(), first.size() * 4}, {&s->instLightSrc, src.data(), src.size() * 4},
                             {&s->instLightObj, obj.data(), obj.size() * 4}, {&s->lightSlot, rank.data(), rank.size() * 4},
                             {&s->lights, nullptr, (size_t)total * 4 * sizeof(float4)}, {&s->instM, nullptr, ni * 48}};
        for (const Upload& u : up) {
            if (int rc = devReserve(*u.buf, u.bytes)) return rc;
            if (u.src) HIP_TRY(hipMemcpy(u.buf->p, u.src, u.bytes, hipMemcpyHostToDevice));
        }
    }
    s->instLightsPrepared = true;
    return PT_OK;
}
// Every build with the bit: the records from the matrices in instM, on `st` (csrc/pt_inst_build.hip).
hipError_t enqueueInstanceLights(pt_scene* s, hipStream_t st) {
    const pt::InstLightIn in{s->dobjs.as<pt_object>(), s->mats.as<float>(), s->instM.as<float>(),
                             s->instLightFirst.as<uint32_t>(), s->instLightSrc.as<uint32_t>(), s->instLightObj.as<uint32_t>(),
                             (uint32_t)s->inst.size(), (uint32_t)s->instLightTotal};
    return pt::instanceLights(in, s->lights.as<float4>(), st);
}

// The full build: pt::buildInstancedTree on the scene's host copies (the materials come back from
// the device in the layout the shading records inline), the arrays uploaded, the scene committed.
int buildInstanced(pt_scene* s, bool lights, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    s->instPrepared = false;
    s->instLightsPrepared = false;
    std::vector<float> mats((size_t)std::max<int64_t>(1, 2 * s->nmat) * 4);
    HIP_TRY(hipMemcpy(mats.data(), s->mats.p, mats.size() * 4, hipMemcpyDeviceToHost));
    pt::InstancedIn in = instancedIn(s);
    in.mats = mats.data();
    const char* rbv = std::getenv("PT_INST_REBRAID");
    in.rebraid = rbv ? std::max(0, std::min(3, std::atoi(rbv))) : 1;
    in.entryBudget = envCount("PT_INST_ENTRIES", 0);
    pt::InstancedTree t;
    int rc = pt::buildInstancedTree(in, t);
    if (rc) return rc;
    // the buffers and what goes into them (src == nullptr: scratch of the later builds, reserved only)
    struct Upload { DevBuf* buf; const void* src; size_t bytes; };
    std::vector<Upload> up = {{&s->wide, t.nodes.data(), t.nodes.size() * 4}, {&s->wprims, t.prims.data(), t.prims.size() * 4},
                              {&s->wshade, t.shade.data(), t.shade.size() * 4}, {&s->winst, t.winst.data(), t.winst.size() * 4}};
    if (s->instDynamic) {   // what the later builds need (rebuildInstancedTop)
        const size_t ni = s->inst.size(), ne = t.entries.size();
        up.insert(up.end(), {{&s->instM, nullptr, ni * 48}, {&s->instOut, nullptr, ni * 48 + ne * 24},
                             {&s->instDesc, t.desc.data(), t.desc.size() * sizeof(pt::InstBoxDesc)},
                             {&s->instSub, t.subBoxes.data(), t.subBoxes.size() * 8},
                             {&s->instPrims, t.entryPrims.data(), t.entryPrims.size() * 4}, {&s->instWprims, nullptr, t.entryPrims.size() * 4},
                             {&s->instRank, t.entryRank.data(), t.entryRank.size() * 4}, {&s->instEntriesDev, t.entries.data(), ne * sizeof(InstEntry)},
                             {&s->instMeshRootDev, t.meshRoot.data(), t.meshRoot.size() * 4}});
        if ((rc = devReserve(s->instErr, 16))) return rc;
        if (!s->wideDev) s->wideDev.reset(new pt::WideDevBuilder);
        HIP_TRY(s->wideDev->reserveTop((int64_t)ne));   // the later builds allocate nothing
    }
    size_t bytes = (size_t)s->nmat * 32;
    for (const Upload& u : up) {
        if ((rc = devReserve(*u.buf, u.bytes))) return rc;
        if (u.src) HIP_TRY(hipMemcpy(u.buf->p, u.src, u.bytes, hipMemcpyHostToDevice));
        bytes += u.bytes;
    }
    std::copy(t.sceneCE, t.sceneCE + 4, s->sceneCE);
    s->mixLim = t.mixLim;
    s->gBits = t.gBits;
    s->wideDepth = t.depth;
    s->wideNodes = (int64_t)(t.nodes.size() / pt::kW8NodeDwords);
    s->instPrimBytes = t.prims.size() * 4;
    s->instShadeBytes = t.shade.size() * 4;
    s->instWinstBytes = t.winst.size() * 4;
    s->wideSource = 3;
    s->wideReady = true;
    s->deviceBytes = bytes;
    if (s->instDynamic) {
        s->instReach = std::move(t.reach);
        s->instEntries = std::move(t.entries);
        s->instMeshRoot = std::move(t.meshRoot);
        s->instTopCap = t.topCap;
        s->instMaxDepthB = t.maxDepthB;
        s->instPrepared = true;
    }
    if (lights) {   // (the tables first: the later builds find every buffer in place)
        if ((rc = prepareInstanceLights(s))) return rc;
        if (s->instLightTotal > 0) {
            std::vector<float> hm(s->inst.size() * 12);
            for (size_t i = 0; i < s->inst.size(); i++) std::memcpy(&hm[i * 12], s->inst[i].m, 48);
            HIP_TRY(hipMemcpy(s->instM.p, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
            StreamWait guard(st);
            HIP_TRY(enqueueInstanceLights(s, st));
            HIP_TRY(hipStreamSynchronize(st));
            guard.ok = true;
        }
    }
    s->instLights = lights;
    s->nLights = lights ? s->instLightTotal : 0;
    s->wideBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->buildMs = s->wideBuildMs;
    s->depth = 0;
    s->built = true;
    return PT_OK;
}

// A dynamic instanced scene's later builds: only what depends on the matrices, on the device, on
// `st`.  The world-to-object rows (instanceRecords: the full build's code, 64 B per instance) and
// the matrices are uploaded; csrc/pt_inst_build.hip computes the instances' exact world boxes and
// the entries' boxes; the instances' boxes (48 B each) are read back for the world box, from which
// the host takes the scene scalars and each mesh's reach exactly as the full build does
// (instanceScalars); then the top level is built in its reserved, zeroed region by the wide
// builder's SAH and collapse stages with one entry per leaf (WideDevBuilder::buildTop) and its
// leaves become instance records (pt::instanceRecords).  The mesh trees, primitive and shading
// records are not touched and nothing is allocated.  The scene's scalars are committed only when
// the build has succeeded.
// *done = false (and PT_OK): a mesh's new reach exceeds the reach its tree was quantised for --
// the caller runs the full build.
int rebuildInstancedTop(pt_scene* s, bool lights, hipStream_t st, bool* done) {
    const auto t0 = std::chrono::steady_clock::now();
    *done = false;
    const int64_t ni = (int64_t)s->inst.size();
    const size_t ne = s->instEntries.size();
    const pt::InstancedIn scn = instancedIn(s);
    pt::InstRecords rec;
    int rc = pt::instanceRecords(scn, rec);
    if (rc) return rc;
    std::vector<float>& hm = s->instHostM;
    std::vector<double>& ibox = s->instHostBox;
    hm.resize((size_t)ni * 12);
    ibox.resize((size_t)ni * 6);
    for (int64_t i = 0; i < ni; i++) std::memcpy(&hm[(size_t)i * 12], s->inst[(size_t)i].m, 48);
    if (!s->instEvents.e0) HIP_TRY(hipEventCreate(&s->instEvents.e0));
    if (!s->instEvents.e1) HIP_TRY(hipEventCreate(&s->instEvents.e1));
    struct { hipEvent_t e0, e1; } ev{s->instEvents.e0, s->instEvents.e1};
    StreamWait guard(st);
    HIP_TRY(hipEventRecord(ev.e0, st));
    HIP_TRY(hipMemcpyAsync(s->instM.p, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->winst.p, rec.winst.data(), rec.winst.size() * 4, hipMemcpyHostToDevice, st));
    double* dibox = s->instOut.as<double>();
    float* debox = reinterpret_cast<float*>(dibox + (size_t)ni * 6);
    const pt::InstBoxIn in{s->dobjs.as<pt_object>(), s->instM.as<float>(), s->instDesc.as<pt::InstBoxDesc>(),
                           s->instSub.as<double>(), ni};
    HIP_TRY(pt::instanceBoxes(in, dibox, debox, st));
    HIP_TRY(hipMemcpyAsync(ibox.data(), dibox, (size_t)ni * 48, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the world box over the instances of non-empty meshes, from it the scalars and the new reach
    double wmn[3] = {INFINITY, INFINITY, INFINITY}, wmx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < ni; i++) {
        if (s->meshCount[(size_t)s->inst[(size_t)i].mesh] == 0) continue;
        for (int r = 0; r < 3; r++) {
            wmn[r] = std::min(wmn[r], ibox[(size_t)i * 6 + (size_t)r]);
            wmx[r] = std::max(wmx[r], ibox[(size_t)i * 6 + 3 + (size_t)r]);
        }
    }
    pt::InstScalars sc;
    std::vector<double> reach;
    pt::instanceScalars(scn, wmn, wmx, rec.w2o, sc, reach);
    for (size_t m = 0; m < reach.size(); m++)
        if (!(reach[m] <= s->instReach[m])) {
            guard.ok = true;
            return PT_OK;
        }
    // the top level, in its reserved region
    HIP_TRY(hipMemsetAsync(s->wide.p, 0, (size_t)s->instTopCap * pt::kW8NodeDwords * 4, st));
    HIP_TRY(hipMemsetAsync(s->instErr.p, 0, 4, st));
    std::string err;
    int topDepth = 0;
    int64_t topSlots = 0;
    const hipError_t e = s->wideDev->buildTop(debox, (int64_t)ne, s->instPrims.as<float4>(), s->instRank.as<uint32_t>(),
                                              s->wide.as<uint32_t>(), s->instWprims.as<uint32_t>(), s->instTopCap, st, err,
                                              topDepth, topSlots);
    if (e != hipSuccess) return fail(err.empty() ? PT_ERR_HIP : PT_ERR_STATE, err.empty() ? hipGetErrorString(e) : err);
    if (topSlots > (int64_t)s->instTopCap) return fail(PT_ERR_STATE, "instanced BVH: top level beyond its reserved node slots");
    HIP_TRY(pt::instanceRecords(s->wide.as<uint32_t>(), (uint32_t)topSlots, s->instWprims.as<uint32_t>(),
                                s->instEntriesDev.as<uint32_t>(), (uint32_t)ne, s->winst.as<float>(),
                                s->instMeshRootDev.as<uint32_t>(), s->instErr.as<uint32_t>(), st));
    // PT_BVH_LIGHTS: the light records of the new matrices (the full build's kernel and tables)
    if (lights && s->instLightTotal > 0) HIP_TRY(enqueueInstanceLights(s, st));
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, s->instErr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.e1, st));
    HIP_TRY(hipEventSynchronize(ev.e1));
    guard.ok = true;
    if (bad) return fail(PT_ERR_STATE, "instanced BVH: malformed top level (flags " + std::to_string(bad) + ")");
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    for (int a = 0; a < 4; a++) s->sceneCE[a] = sc.ce[a];
    s->mixLim = sc.mixLim;
    s->wideDepth = topDepth + 1 + s->instMaxDepthB + 1;
    s->wideSource = 4;
    s->wideReady = true;
    s->instLights = lights;
    s->nLights = lights ? s->instLightTotal : 0;
    s->buildMs = (double)ms;
    s->wideBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->depth = 0;
    if (wideStackFor(s->wideDepth) < 0) return fail(PT_ERR_STATE, "instanced BVH too deep");
    s->built = true;
    *done = true;
    return PT_OK;
}

int setDevice(int dev) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PT_ERR_NODEVICE, "no HIP device visible (the library has no CPU fallback)");
    if (dev < 0 || dev >= count) return fail(PT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(dev));
    return PT_OK;
}

// The AHEAD instantiations that exist: triangle-only kernels at the stacks where a wave's 768 more
// bytes of LDS leave five waves per SIMD (the 24-entry stack's 20 waves would need 165 KB of 160).
template <int S, bool TRI>
constexpr bool kAheadFor = TRI && S <= 16;
static_assert(kAheadFor<8, true> && kAheadFor<16, true> && !kAheadFor<24, true> && pt::aheadStack(8) && pt::aheadStack(16) &&
                  !pt::aheadStack(24), "the launch plan's aheadStack (host/pt_render_plan.hpp) names the AHEAD instantiations");
// Sample mode on a flat scene.  TRI = P.tri: the triangle-only instantiations.
template <int S, bool LIT, bool TRI>
void launchSampleWideFlat(const RenderParams& P, hipStream_t st) {
    if constexpr (LIT) {   // (NEE launches are LIT: a sampled light is an emissive material)
        if (P.nLights > 0) {
            if (P.mis) PT_LAUNCH_WF(P.nwaves, S, true, true, false, true, true, true, TRI);
            else PT_LAUNCH_WF(P.nwaves, S, true, true, false, true, true, false, TRI);
            return;
        }
    }
    if constexpr (kAheadFor<S, TRI>) {   // (P.ahead: set for these instantiations only, pt_render_ex)
        if (P.ahead) {
            PT_LAUNCH_WF(P.nwaves, S, true, true, false, LIT, false, false, TRI, true);
            return;
        }
    }
    PT_LAUNCH_WF(P.nwaves, S, true, true, false, LIT, false, false, TRI);
}
// LIT = P.lit (dispatchRender): the kernels with the emissive exit and the scene's own sky
template <int S, bool LIT>
void launchRenderWide(const RenderParams& P, hipStream_t st) {
    if (P.S.winst) {   // an instanced scene's two-level tree
        if constexpr (LIT) {   // (built with PT_BVH_LIGHTS: the NEE / MIS kernels, as below)
            if (P.nLights > 0) {
                if (P.pixAcc && P.mis) PT_LAUNCH_WF(P.nwaves, S, true, true, true, true, true, true);
                else if (P.pixAcc) PT_LAUNCH_WF(P.nwaves, S, true, true, true, true, true);
                else if (P.mis) PT_LAUNCH_WF(P.compatGrid, S, false, true, true, true, true, true);
                else PT_LAUNCH_WF(P.compatGrid, S, false, true, true, true, true);
                return;
            }
        }
        if (P.pixAcc) PT_LAUNCH_WF(P.nwaves, S, true, true, true, LIT);
        else PT_LAUNCH_WF(P.compatGrid, S, false, true, true, LIT);
        return;
    }
    if (P.pixAcc) {
        P.tri ? launchSampleWideFlat<S, LIT, true>(P, st) : launchSampleWideFlat<S, LIT, false>(P, st);
    } else {
        pt::launchCompatWide(S, &P, st);   // (its own translation unit, pt_compat.hip; reads P.lit, P.nLights, P.tri)
    }
}
template <int S, bool LIT>
void launchRender(const RenderParams& P, hipStream_t st) {
    if (P.kernel == PT_KERNEL_WAVEFRONT && P.pixAcc)
        PT_LAUNCH_WF(P.nwaves, S, true, false, false, LIT);
    else if (P.kernel == PT_KERNEL_WAVEFRONT)
        PT_LAUNCH_WF(P.compatGrid, S, false, false, false, LIT);
    else if (LIT && P.nLights > 0 && P.mis && P.pixAcc) PT_LAUNCH_SIMPLE(P.ntiles, S, true, LIT, LIT, LIT);
    else if (LIT && P.nLights > 0 && P.mis) PT_LAUNCH_SIMPLE(P.ntiles, S, false, LIT, LIT, LIT);
    else if (LIT && P.nLights > 0 && P.pixAcc) PT_LAUNCH_SIMPLE(P.ntiles, S, true, LIT, LIT);
    else if (LIT && P.nLights > 0) PT_LAUNCH_SIMPLE(P.ntiles, S, false, LIT, LIT);
    else if (P.pixAcc) PT_LAUNCH_SIMPLE(P.ntiles, S, true, LIT);
    else PT_LAUNCH_SIMPLE(P.ntiles, S, false, LIT);
}
template <int S, bool WIDE, bool INST = false, bool SAMPLE = true, bool TRI = false, bool AHEAD = false>
int wavesPerCU(int& n) {
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &n, reinterpret_cast<const void*>(&renderKernelWF<S, SAMPLE, WIDE, INST, false, false, false, TRI, AHEAD>), kWave, 0));
    return PT_OK;
}
// A run-time stack size as a compile-time constant: f(std::integral_constant<int, N>) for the N
// of `Ns` that equals `stack`; false when there is none (an unsupported depth).  The lists are
// wideStackFor's and stackFor's, so exactly those kernels are instantiated.
template <int... Ns, class F>
bool withStack(int stack, F f) {
    return ((stack == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...);
}
template <class F>
bool withWideStack(int stack, F f) { return withStack<8, 16, 24>(stack, f); }
template <class F>
bool withBinStack(int stack, F f) { return withStack<16, 24, 32, 48, 64, 80>(stack, f); }

// Waves per CU of the render kernel a launch runs: its occupancy (sample mode launches exactly the
// waves that fit; compat launches do not ask).  Asked of the kernel without LIT: its LIT twin has
// the same LDS and waves-per-SIMD attribute, so the same occupancy (DESIGN.md's resource table).
// The compat wide kernels live in pt_compat.hip's
// translation unit.  tri: the launch runs a TRI instantiation (RenderParams::tri), which is asked.
int persistentWavesPerCU(int stack, int kernel, int& n, bool inst, bool sample, bool nee, bool mis, bool tri, bool ahead) {
    const bool wide = kernel == PT_KERNEL_WIDE;
    if (ahead) {   // (wide, sample, flat, tri, no NEE: the AHEAD kernels hold the slots' LDS, so they are asked themselves)
        int rc = PT_OK;
        const bool ok = withStack<8, 16>(stack, [&](auto N) { rc = wavesPerCU<decltype(N)::value, true, false, true, true, true>(n); });
        if (!ok) return fail(PT_ERR_STATE, "unsupported wide BVH depth");
        return rc;
    }
    if (wide && sample && nee) {   // the NEE and MIS kernels hold more LDS per wave: asked of themselves
        int rc = PT_OK;
        const bool ok = withWideStack(stack, [&](auto N) {
            constexpr int K = decltype(N)::value;
            const void* k = inst ? (mis ? reinterpret_cast<const void*>(&renderKernelWF<K, true, true, true, true, true, true>)
                                        : reinterpret_cast<const void*>(&renderKernelWF<K, true, true, true, true, true>))
                          : tri  ? (mis ? reinterpret_cast<const void*>(&renderKernelWF<K, true, true, false, true, true, true, true>)
                                        : reinterpret_cast<const void*>(&renderKernelWF<K, true, true, false, true, true, false, true>))
                                 : (mis ? reinterpret_cast<const void*>(&renderKernelWF<K, true, true, false, true, true, true>)
                                        : reinterpret_cast<const void*>(&renderKernelWF<K, true, true, false, true, true>));
            const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, kWave, 0);
            if (e != hipSuccess) rc = fail(PT_ERR_HIP, std::string("hipOccupancyMaxActiveBlocksPerMultiprocessor: ") + hipGetErrorString(e));
        });
        if (!ok) return fail(PT_ERR_STATE, "unsupported wide BVH depth");
        return rc;
    }
    if (wide && !inst && !sample)
        return pt::compatWideWavesPerCU(stack, tri, n) ? fail(PT_ERR_STATE, "unsupported wide BVH depth") : PT_OK;
    int rc = PT_OK;
    const bool ok = wide ? withWideStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        rc = !inst ? (tri ? wavesPerCU<K, true, false, true, true>(n) : wavesPerCU<K, true>(n)) : sample ? wavesPerCU<K, true, true>(n) : wavesPerCU<K, true, true, false>(n);
    }) : withBinStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        rc = sample ? wavesPerCU<K, false>(n) : wavesPerCU<K, false, false, false>(n);
    });
    if (!ok) return fail(PT_ERR_STATE, !wide ? "unsupported BVH depth" : inst ? "unsupported instanced BVH depth" : "unsupported wide BVH depth");
    return rc;
}
// persistentWavesPerCU, asked once per (device, kernel instantiation) and process: its own argument
// list after the device, so the cache's key and the query cannot drift apart.  Stacks of 8, 16 and 24
// on devices 0..15 have a slot; the binary tree's deeper stacks (32 .. 80) have none and ask on every call.
int cachedWavesPerCU(int device, int stack, int kernel, int& n, bool inst, bool sample, bool nee, bool mis, bool tri, bool ahead) {
    static std::atomic<int> cached[16][2][2][2][3][3][2][2];   // [device][sample][instanced][wide][stack 8, 16, 24][blind, nee, mis][tri][ahead]
    const bool small = stack <= 24 && stack % 8 == 0 && device >= 0 && device < 16;
    std::atomic<int>* c = small ? &cached[device][sample ? 1 : 0][inst ? 1 : 0][kernel == PT_KERNEL_WIDE ? 1 : 0][stack / 8 - 1]
                                         [mis ? 2 : nee ? 1 : 0][tri ? 1 : 0][ahead ? 1 : 0] : nullptr;
    const int known = c ? c->load(std::memory_order_relaxed) : 0;
    if (known > 0) {
        n = known;
        return PT_OK;
    }
    if (int r = persistentWavesPerCU(stack, kernel, n, inst, sample, nee, mis, tri, ahead)) return r;
    if (c) c->store(n, std::memory_order_relaxed);
    return PT_OK;
}
int dispatchRender(int stack, const RenderParams& P, hipStream_t st) {
    const bool wide = P.kernel == PT_KERNEL_WIDE;
    const bool ok = wide ? withWideStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        P.lit ? launchRenderWide<K, true>(P, st) : launchRenderWide<K, false>(P, st);
    }) : withBinStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        P.lit ? launchRender<K, true>(P, st) : launchRender<K, false>(P, st);
    });
    if (!ok) return fail(PT_ERR_STATE, wide ? "unsupported wide BVH depth" : "unsupported BVH depth");
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// The ray queries' grid: at most 32 one-wave blocks per CU (the grid-stride kernels stride over
// the batch, the queued ones take rays from its queue).
unsigned queryBlocks(int64_t n) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    return (unsigned)std::min<int64_t>((n + kWave - 1) / kWave, (int64_t)cus * 32);
}
// pt_trace_closest: the queued kernel of either tree; PT_TRACE_STRIDE=1: the grid-stride one (A/B).
int dispatchTrace(int stack, bool wide, const DevScene& S, const pt_ray* r, int64_t n, float tmin, float tmax,
                  pt_hit* h, unsigned long long* cnt, hipStream_t st) {
    const char* strideEnv = std::getenv("PT_TRACE_STRIDE");
    const bool stride = strideEnv && std::atoi(strideEnv) != 0;
    const auto launch = [&](auto* kernel) { kernel<<<queryBlocks(n), kWave, 0, st>>>(S, r, n, tmin, tmax, h, cnt); };
    const bool ok = wide ? withWideStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        if (S.winst) launch(stride ? traceKernelWide<K, true> : traceKernelWideQ<K, true>);
        else launch(stride ? traceKernelWide<K, false> : traceKernelWideQ<K, false>);
    }) : withBinStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        launch(stride ? traceKernel<K> : traceKernelQ<K>);
    });
    if (!ok)   // (the texts of the former tables: "instanced" only ever appeared on the grid-stride path)
        return fail(PT_ERR_STATE, !wide ? "unsupported BVH depth"
                                        : stride && S.winst ? "unsupported instanced BVH depth" : "unsupported wide BVH depth");
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
// pt_render_aov: the queued wide kernel over the film's n pixels.
int dispatchAov(int stack, const DevScene& S, const AovCam& cam, int64_t n, float4* out, unsigned long long* cnt,
                hipStream_t st) {
    const bool ok = withWideStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        const auto launch = [&](auto* kernel) { kernel<<<queryBlocks(n), kWave, 0, st>>>(S, cam, n, out, cnt); };
        launch(S.winst ? aovKernelWideQ<K, true> : aovKernelWideQ<K, false>);
    });
    if (!ok) return fail(PT_ERR_STATE, "unsupported wide BVH depth");
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
// pt_trace_occluded: the queued kernel of either tree.
int dispatchOccluded(int stack, bool wide, const DevScene& S, const pt_ray* r, int64_t n, float tmin, float tmax,
                     const float* rt, uint8_t* occ, unsigned long long* cnt, hipStream_t st) {
    const auto launch = [&](auto* kernel) { kernel<<<queryBlocks(n), kWave, 0, st>>>(S, r, n, tmin, tmax, rt, occ, cnt); };
    const bool ok = wide ? withWideStack(stack, [&](auto N) {
        constexpr int K = decltype(N)::value;
        launch(S.winst ? occludedKernelWideQ<K, true> : occludedKernelWideQ<K, false>);
    }) : withBinStack(stack, [&](auto N) { launch(occludedKernelQ<decltype(N)::value>); });
    if (!ok) return fail(PT_ERR_STATE, wide ? "unsupported wide BVH depth" : "unsupported BVH depth");
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// (Re)initialise every stream of the film to curand_init(seed, pixel, 0), asynchronously.
int filmInit(pt_film* f, hipStream_t st) {
    if (f->npix <= 0) return PT_OK;
    uint32_t* b = f->state.as<uint32_t>();
    const int64_t np = f->npix;
    rngInitKernel<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(b, b + np, b + 2 * np, b + 3 * np, b + 4 * np, b + 5 * np,
                                                                 f->jumps.as<uint32_t>(), f->seed, f->width, f->nrows,
                                                                 f->stripe_h, f->nparts, f->part);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

DevScene devScene(const pt_scene* s) {
    DevScene S;
    S.nodes = s->nodes.as<float4>();
    S.prims = s->prims.as<float4>();
    S.shade = s->shade.as<float4>();
    S.mats = s->mats.as<float4>();
    S.wnodes = s->wide.as<float4>();
    S.wprims = s->wprims.as<float4>();
    S.wshade = s->wshade.as<float4>();
    S.wbox = s->wbox.as<float4>();
    S.rankOf = s->rankOf.as<uint32_t>();
    S.iparent = s->iparent.as<int>();
    S.err = reinterpret_cast<unsigned int*>(s->counters.as<unsigned long long>() + 7);
    S.nprims = (int)s->nobj;
    S.hasSpheres = s->hasSpheres ? 1 : 0;
    S.cx = s->sceneCE[0]; S.cy = s->sceneCE[1]; S.cz = s->sceneCE[2]; S.ext = s->sceneCE[3];
    S.mixLim = s->mixLim;
    S.winst = s->instanced ? s->winst.as<float4>() : nullptr;
    S.gBits = s->gBits;
    return S;
}

// Algorithmic bytes: per binary node visit both child boxes + refs (56 B), per
// wide node visit the 80-B compressed record (8 child boxes, refs, frame); 40 B per triangle
// test, 20 B per sphere test.
void fillStats(pt_stats* st, const unsigned long long c[5], double ms, bool wide = false) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->rays = c[0];
    st->node_visits = c[1];
    st->box_tests = (wide ? 8 : 2) * c[1];
    st->tri_tests = c[2];
    st->sphere_tests = c[3];
    st->paths = c[4];
    st->kernel_ms = ms;
    st->algo_bytes = (wide ? 80ull : 56ull) * c[1] + 40ull * c[2] + 20ull * c[3];
}

// Diagnostics of the wavefront scheduler (PT_ITER_STATS=1; the per-step counters need a PT_DIAG build).
void printIterStats(const unsigned long long* c, bool wide) {
    if (c[8] + c[9] + c[10] > 0)
        std::fprintf(stderr, "[pt] iterations node %llu leaf %llu shade %llu | lanes/iter node %.1f leaf %.1f "
                     "shade %.1f\n", c[8], c[9], c[10], (double)c[1] / std::max(1ull, c[8]),
                     (double)c[11] / std::max(1ull, c[9]), (double)c[0] / std::max(1ull, c[10]));
    if (c[12] + c[13] + c[14] > 0)
        std::fprintf(stderr, "[pt] cycles/iteration node %.0f leaf %.0f shade %.0f | share node %.3f leaf %.3f "
                     "shade %.3f\n", (double)c[12] / std::max(1ull, c[8]), (double)c[13] / std::max(1ull, c[9]),
                     (double)c[14] / std::max(1ull, c[10]), (double)c[12] / (double)(c[12] + c[13] + c[14]),
                     (double)c[13] / (double)(c[12] + c[13] + c[14]), (double)c[14] / (double)(c[12] + c[13] + c[14]));
    if (wide && c[8] > 0)
        std::fprintf(stderr, "[pt] wide queries repeated in the reference order: %llu (lanes x steps; %llu for a final "
                     "hit whose box the ray misses); NODE steps: "
                     "lanes waiting on primitives with nodes left %.1f, lanes without NODE work %.1f\n", c[20], c[23],
                     (double)c[21] / std::max(1ull, c[8]), (double)c[22] / std::max(1ull, c[8]));
    if (wide && c[9] > 0)
        std::fprintf(stderr, "[pt] LEAF: lanes testing one primitive per step %.1f; tests in groups that were parked "
                     "%llu (%.3f)\n", (double)c[25] / std::max(1ull, c[9]), c[27],
                     (double)c[27] / std::max(1ull, c[2] + c[3]));
    if (c[15] > 0)
        std::fprintf(stderr, "[pt] loop head (choice of the step kind) cycles/iteration %.0f\n",
                     (double)c[15] / std::max(1ull, c[8] + c[9] + c[10]));
    if (c[14] > 0)
        std::fprintf(stderr, "[pt] SHADE cycles/iteration: shading %.0f tasks %.0f new-path %.0f ray-start %.0f\n",
                     (double)c[16] / std::max(1ull, c[10]), (double)c[17] / std::max(1ull, c[10]),
                     (double)c[18] / std::max(1ull, c[10]), (double)c[19] / std::max(1ull, c[10]));
    if (c[26] > 0)
        std::fprintf(stderr, "[pt] SHADE unit-sphere trial-loop iterations %llu (%.2f per SHADE step)\n", c[26],
                     (double)c[26] / std::max(1ull, c[10]));
}

// The film's last render -> pt_stats: waits for its counters (copied to pinned memory in stream
// order, event ev2) and takes the kernels' time from its events; reports a tripped traversal guard.
int filmStats(pt_film* f, pt_stats* stats) {
    if (!f->rendered) return fail(PT_ERR_STATE, "pt_film_stats: no render on this film yet");
    HIP_TRY(hipEventSynchronize(f->ev2));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, f->ev0, f->ev1));
    const unsigned long long* c = f->hostCounters;
    fillStats(stats, c, ms, f->lastWide);
    if (std::getenv("PT_ITER_STATS")) printIterStats(c, f->lastWide);
    if (c[7]) return fail(PT_ERR_STATE, "traversal guard tripped (corrupt BVH), flags " + std::to_string(c[7]));
    return PT_OK;
}

// ------------------------------------------------------------------ pt_render_ex's stages
// What the launch plan (host/pt_render_plan.hpp) reads of the scene, the film and the call.
pt::RenderFacts renderFacts(const pt_scene* s, const pt_film* f, const pt_camera* cam, int spp, int max_depth,
                            const pt_render_opts* opts) {
    pt::RenderFacts F;
    F.instanced = s->instanced;
    F.instLights = s->instLights;
    F.hasSpheres = s->hasSpheres;
    F.hasEmissive = s->hasEmissive;
    F.lambertOnly = s->lambertOnly;
    F.wideReady = s->wideReady;
    F.haveWtris = s->haveWtris;
    F.nobj = s->nobj;
    F.nLights = s->nLights;
    F.depth = s->depth;
    F.wideDepth = s->wideDepth;
    std::memcpy(F.sceneCE, s->sceneCE, sizeof(F.sceneCE));
    std::memcpy(F.skyH, s->skyH, sizeof(F.skyH));
    std::memcpy(F.skyZ, s->skyZ, sizeof(F.skyZ));
    F.width = f->width;
    F.height = f->height;
    F.nrows = f->nrows;
    F.stripe_h = f->stripe_h;
    F.npix = f->npix;
    F.haveOrder = f->haveOrder;
    F.framesSinceCost = f->framesSinceCost;
    F.critK = f->critK;
    F.accumSamples = f->accumSamples;
    F.cam = cam;
    F.spp = spp;
    F.max_depth = max_depth;
    F.opts = opts;
    return F;
}

// What one call's stages hand on beside the plan.
struct RenderCall {
    hipStream_t st = 0;
    void* dst = nullptr;          // the frame on the device: the caller's `out`, or the film's staging copy
    size_t outBpp = 12;
    int nwaves = 0;               // sample mode: persistent waves
    bool newAccum = false;        // this call allocated the running sums: they are cleared with the frame
    const char* timesPath = nullptr;   // PT_WAVE_TIMES (diagnostic): per-wave timestamps
    size_t timeSlots = 0;         // = grid size
    DevBuf dtimes;
};

// Film resources, allocated once and reused by every later render (no hipMalloc / hipFree,
// which synchronise the device, in the per-frame path).  Enqueues nothing.
int reserveFilm(const pt_scene* s, pt_film* f, const pt::RenderOptions& o, const pt::RenderPlan& plan, bool on_dev, RenderCall& c) {
    int rc = PT_OK;
    const int64_t np = f->npix;
    if (!f->ev0) {
        HIP_TRY(hipEventCreate(&f->ev0));
        HIP_TRY(hipEventCreate(&f->ev1));
        HIP_TRY(hipEventCreateWithFlags(&f->ev2, hipEventDisableTiming));
    }
    if (!f->counters.p && (rc = devAlloc(f->counters, kNumCounters * sizeof(unsigned long long)))) return rc;
    if (!f->hostCounters) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&f->hostCounters),
                                                kNumCounters * sizeof(unsigned long long), hipHostMallocDefault));
    if (!on_dev) {
        if ((rc = devReserve(f->staging, (size_t)std::max<int64_t>(1, np) * c.outBpp))) return rc;
        c.dst = f->staging.p;
    }
    const size_t ntl = (size_t)std::max(1, plan.ntiles);
    if (!f->tileCost.p) {
        if ((rc = devAlloc(f->tileCost, ntl * 4)) || (rc = devAlloc(f->tileOrder, ntl * 4)) ||
            (rc = devAlloc(f->tileXY, ntl * 4)) || (rc = devAlloc(f->tileXYId, ntl * 4)))
            return rc;
        f->haveOrder = false;
    }
    if (!f->cus) {
        if (hipDeviceGetAttribute(&f->cus, hipDeviceAttributeMultiprocessorCount, f->device) != hipSuccess)
            f->cus = 256;
        f->cus = std::max(f->cus, 1);
    }
    if (plan.critOn && (rc = devReserve(f->pixRays, (size_t)np * 4))) return rc;
    if (plan.sample) {
        if ((rc = devReserve(f->pixAcc, (size_t)np * 32))) return rc;   // {x, y, z, rays} per pixel
        if (!f->taskCounter.p && (rc = devAlloc(f->taskCounter, 64))) return rc;
        int perCU = 0;
        if ((rc = cachedWavesPerCU(f->device, plan.stack, o.kernel, perCU, s->instanced, plan.sample, o.nee, o.mis, plan.tri != 0,
                                   plan.ahead != 0)))
            return rc;
        if ((rc = pt::persistentWaves(f->cus, perCU, plan.ntasks, c.nwaves))) return rc;
        if (std::getenv("PT_ITER_STATS"))
            std::fprintf(stderr, "[pt] persistent waves %d (%d per CU, stack %d)\n", c.nwaves, perCU, plan.stack);
    }
    if (plan.spillEntries > 0 &&
        (rc = devReserve(f->stackSpill, plan.stackSpillBytes(plan.sample ? (size_t)c.nwaves : (size_t)plan.compatGrid))))
        return rc;
    if (plan.rawOut && !f->sums.p && (rc = devAlloc(f->sums, (size_t)np * 12))) return rc;
    if (o.accumulate && !f->accum.p) {
        if ((rc = devAlloc(f->accum, (size_t)std::max<int64_t>(1, np) * 12))) return rc;
        f->accumSamples = 0;
        c.newAccum = true;
    }
    c.timesPath = std::getenv("PT_WAVE_TIMES");
    c.timeSlots = plan.sample ? (size_t)c.nwaves : (o.kernel != PT_KERNEL_SIMPLE ? (size_t)std::max(1, plan.compatGrid) : ntl);
    if (c.timesPath && *c.timesPath && o.kernel != PT_KERNEL_SIMPLE && (rc = devAlloc(c.dtimes, c.timeSlots * 24))) return rc;
    return PT_OK;
}

// The kernels' argument: every field, in the struct's order.
void fillRenderParams(RenderParams& P, const pt_scene* s, const pt_film* f, const pt_camera* cam, int spp, int max_depth,
                      const pt::RenderOptions& o, const pt::RenderPlan& plan, const RenderCall& c) {
    const int64_t np = f->npix;
    const bool tileOrder = o.lpt && f->haveOrder;
    P.S = devScene(s);
    P.S.err = reinterpret_cast<unsigned int*>(f->counters.as<unsigned long long>() + 7);
    if (plan.triRecords) P.S.wprims = s->wtris.as<float4>();
    P.cam.pos = make_float3(cam->origin[0], cam->origin[1], cam->origin[2]);
    P.cam.ll = make_float3(cam->lower_left[0], cam->lower_left[1], cam->lower_left[2]);
    P.cam.hor = make_float3(cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]);
    P.cam.ver = make_float3(cam->vertical[0], cam->vertical[1], cam->vertical[2]);
    P.cam.right = make_float3(cam->right[0], cam->right[1], cam->right[2]);
    P.cam.up = make_float3(cam->up[0], cam->up[1], cam->up[2]);
    P.cam.lens = cam->lens_radius;
    uint32_t* b = f->state.as<uint32_t>();
    P.sd = b; P.s0 = b + np; P.s1 = b + 2 * np; P.s2 = b + 3 * np; P.s3 = b + 4 * np; P.s4 = b + 5 * np;
    P.out = plan.rawOut ? f->sums.as<float>() : static_cast<float*>(c.dst);
    P.counters = f->counters.as<unsigned long long>();
    P.width = f->width;
    P.nrows = f->nrows;
    P.stripe_h = f->stripe_h;
    P.nparts = f->nparts;
    P.part = f->part;
    P.tiles_x = plan.tiles_x;
    P.ntiles = plan.ntiles;
    P.spp = spp;
    P.max_depth = max_depth;
    P.invW = 1.0f / (float)f->width;    // main.cu:281
    P.invH = 1.0f / (float)f->height;
    P.invSpp = 1.0f / (float)spp;
    P.leafBatch = plan.leafBatch;
    P.shadeBatch = plan.shadeBatch;
    P.nodeMin = plan.nodeMin;
    P.kernel = o.kernel;
    P.waveTimes = c.dtimes.as<unsigned long long>();
    P.tileOrder = tileOrder ? f->tileOrder.as<int>() : nullptr;
    // sample mode: the launch order decoded per slot (tileXYKernel; the ordered table follows each sort)
    P.tileXY = !plan.sample ? nullptr : tileOrder ? f->tileXY.as<uint32_t>() : f->tileXYId.as<uint32_t>();
    P.nblocksShift = plan.nblocksShift;
    P.tileCost = f->tileCost.as<unsigned>();
    P.prioTiles = plan.prioTiles;
    P.prioLevel = plan.prioLevel;
    P.nblocks = plan.nblocks;
    P.block = plan.block;
    P.group = 1;
    P.span = plan.span;
    P.ngroups = plan.ngroups;
    P.pixAcc = plan.sample ? f->pixAcc.as<unsigned long long>() : nullptr;
    P.taskCounter = plan.sample ? f->taskCounter.as<unsigned>() : nullptr;
    P.stackSpill = plan.spillEntries > 0 ? f->stackSpill.as<uint32_t>() : nullptr;
    P.ntasks = plan.ntasks;
    P.nwaves = c.nwaves;
    P.seed0 = (uint32_t)f->seed;
    P.seed1 = (uint32_t)(f->seed >> 32);
    P.sampleBase = plan.sampleBase;
    P.measureCost = plan.measureCost;
    P.camFar = plan.camFar;
    P.rawOut = plan.rawOut;
    P.stripeShift = plan.stripeShift;
    P.blockShift = plan.blockShift;
    P.splitTiles = plan.splitTiles;
    P.splitWays = plan.splitWays;
    P.compatGrid = plan.compatGrid;
    P.nCrit = plan.nCrit;
    P.critLanes = plan.critLanes;
    P.critWaves = plan.critWaves;
    P.critList = plan.nCrit > 0 ? f->pixSorted.as<uint32_t>() : nullptr;
    P.critFlag = plan.nCrit > 0 ? f->critFlag.as<uint8_t>() : nullptr;
    P.pixRays = plan.critOn ? f->pixRays.as<uint32_t>() : nullptr;
    P.skyH = make_float3(s->skyH[0], s->skyH[1], s->skyH[2]);
    P.skyZ = make_float3(s->skyZ[0], s->skyZ[1], s->skyZ[2]);
    P.lit = plan.lit;
    P.lights = o.nee ? s->lights.as<float4>() : nullptr;
    P.nLights = o.nee ? (int)s->nLights : 0;
    P.mis = o.mis ? 1 : 0;
    P.lightSlot = o.mis ? s->lightSlot.as<uint32_t>() : nullptr;   // (instanced: the ranks by shading index)
    P.instLightFirst = o.mis && s->instanced ? s->instLightFirst.as<uint32_t>() : nullptr;
    P.tri = plan.tri;
    P.ahead = plan.ahead;
}

// The frame on the stream: the buffers' clears, the render kernel between the film's events, the
// resolve pass, the counters' copy.  From its first event on the film describes this render.
int enqueueFrame(pt_film* f, const RenderParams& P, int spp, const pt::RenderOptions& o, const pt::RenderPlan& plan,
                 const RenderCall& c) {
    int rc = PT_OK;
    hipStream_t st = c.st;
    const int64_t np = f->npix;
    const size_t ntl = (size_t)std::max(1, plan.ntiles);
    HIP_TRY(hipMemsetAsync(f->counters.p, 0, kNumCounters * sizeof(unsigned long long), st));
    if (plan.sample) {
        HIP_TRY(hipMemsetAsync(f->pixAcc.p, 0, (size_t)np * 32, st));
        HIP_TRY(hipMemsetAsync(f->taskCounter.p, 0, 4, st));
        f->framesSinceCost = plan.measureCost ? 0 : f->framesSinceCost + 1;
        if (plan.measureCost) HIP_TRY(hipMemsetAsync(f->tileCost.p, 0, ntl * 4, st));
    }
    if (c.newAccum) HIP_TRY(hipMemsetAsync(f->accum.p, 0, (size_t)std::max<int64_t>(1, np) * 12, st));
    if (plan.sample && !P.tileOrder && !f->haveXYId) {   // the identity order decoded, once
        tileXYKernel<<<(unsigned)((ntl + 255) / 256), 256, 0, st>>>(nullptr, (int)ntl, P.tiles_x, f->tileXYId.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        f->haveXYId = true;
    }
    if (!plan.sample && o.kernel != PT_KERNEL_SIMPLE && P.ntiles > 0)   // (tile costs: atomicMax of the tile's waves)
        HIP_TRY(hipMemsetAsync(f->tileCost.p, 0, ntl * 4, st));
    if (P.waveTimes) HIP_TRY(hipMemsetAsync(c.dtimes.p, 0, c.timeSlots * 24, st));
    // From here on the film describes this render (pt_film_stats reads it).
    f->rendered = false;
    f->lastWide = o.kernel == PT_KERNEL_WIDE;
    HIP_TRY(hipEventRecord(f->ev0, st));
    if (P.ntiles > 0 && (rc = dispatchRender(plan.stack, P, st))) return rc;
    if (plan.resolve) {
        const float inv = o.accumulate ? 1.0f / (float)(f->accumSamples + spp) : P.invSpp;
        resolveKernel<<<(unsigned)((np + 255) / 256), 256, 0, st>>>(f->sums.as<float>(), plan.sample ? P.pixAcc : nullptr,
                                                                     o.accumulate ? f->accum.as<float>() : nullptr,
                                                                     inv, o.fmt, c.dst, np,
                                                                     P.measureCost ? f->tileCost.as<unsigned>() : nullptr,
                                                                     f->width, P.tiles_x, envInt("PT_TILE_KEY_MAX", 1));
        HIP_TRY(hipGetLastError());
    }
    if (o.accumulate) f->accumSamples += spp;
    HIP_TRY(hipEventRecord(f->ev1, st));
    // the counters to pinned host memory, in stream order (pt_film_stats waits for ev2 only)
    HIP_TRY(hipMemcpyAsync(f->hostCounters, f->counters.p, kNumCounters * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(f->ev2, st));
    f->rendered = true;
    return PT_OK;
}

// Ids 0 .. n-1 by descending cost (keys ~cost, ascending: tileKeyKernel), equal costs by ascending
// id: a stable radix sort on the device.
int sortByCostDescending(const DevBuf& cost, DevBuf& keys, DevBuf& keys2, DevBuf& ids, DevBuf& sorted, DevBuf& temp, size_t n,
                         hipStream_t st) {
    int rc = PT_OK;
    if ((rc = devReserve(keys, n * 4)) || (rc = devReserve(keys2, n * 4)) || (rc = devReserve(ids, n * 4))) return rc;
    tileKeyKernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(cost.as<unsigned>(), keys.as<uint32_t>(), ids.as<uint32_t>(), (int)n);
    HIP_TRY(hipGetLastError());
    return sortPairs(temp, keys.as<uint32_t>(), keys2.as<uint32_t>(), ids.as<uint32_t>(), sorted.as<uint32_t>(), n, 32, st);
}

// What the next launches start with: the longest tiles first, and (compat, wide kernel) the critical
// pixels -- the K longest chains of this launch.
int sortNextLaunch(pt_film* f, const pt::RenderOptions& o, const pt::RenderPlan& plan, hipStream_t st) {
    int rc = PT_OK;
    if (plan.sortTiles) {
        const size_t ntl = (size_t)plan.ntiles;
        if ((rc = sortByCostDescending(f->tileCost, f->tileKeys, f->tileKeys2, f->tileIds, f->tileOrder, f->sortTemp, ntl, st)))
            return rc;
        tileXYKernel<<<(unsigned)((ntl + 255) / 256), 256, 0, st>>>(f->tileOrder.as<uint32_t>(), (int)ntl, plan.tiles_x,
                                                                    f->tileXY.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        f->haveOrder = true;
    }
    if (plan.critOn) {
        const size_t n = (size_t)f->npix;
        const int64_t K = std::min<int64_t>(envCount("PT_CRIT_PIXELS", pt::kCritPixels), f->npix);
        if ((rc = devReserve(f->pixSorted, n * 4)) || (rc = devReserve(f->critFlag, n))) return rc;
        if ((rc = sortByCostDescending(f->pixRays, f->pixKeys, f->pixKeys2, f->pixIds, f->pixSorted, f->critTemp, n, st))) return rc;
        HIP_TRY(hipMemsetAsync(f->critFlag.p, 0, n, st));
        critFlagKernel<<<(unsigned)((K + 255) / 256), 256, 0, st>>>(f->pixSorted.as<uint32_t>(), (int)K,
                                                                   f->critFlag.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        f->critK = (int)K;
    }
    return PT_OK;
}

// Diagnostics, each with a wait for the stream: PT_CHECK_ORDER (the launch order just sorted must be a
// permutation of the tiles, by descending cost) and PT_WAVE_TIMES (the frame's per-wave timestamps to a file).
int dumpDiagnostics(pt_film* f, const pt::RenderPlan& plan, const RenderCall& c) {
    if (plan.sortTiles && std::getenv("PT_CHECK_ORDER")) {
        const size_t ntl = (size_t)plan.ntiles;
        std::vector<uint32_t> ord(ntl), cst(ntl);
        HIP_TRY(hipStreamSynchronize(c.st));
        HIP_TRY(hipMemcpy(ord.data(), f->tileOrder.p, ntl * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cst.data(), f->tileCost.p, ntl * 4, hipMemcpyDeviceToHost));
        std::vector<uint8_t> seen(ntl, 0);
        size_t dup = 0, bad = 0, unsorted = 0;
        for (size_t k = 0; k < ntl; k++) {
            if (ord[k] >= ntl) { bad++; continue; }
            if (seen[ord[k]]++) dup++;
            if (k && ord[k - 1] < ntl && cst[ord[k - 1]] < cst[ord[k]]) unsorted++;
        }
        std::fprintf(stderr, "[pt] tile order check: %zu tiles, %zu out of range, %zu duplicates, %zu unsorted pairs\n",
                     ntl, bad, dup, unsorted);
    }
    if (c.dtimes.p) {
        HIP_TRY(hipStreamSynchronize(c.st));
        std::vector<unsigned long long> t(c.timeSlots * 3);
        HIP_TRY(hipMemcpy(t.data(), c.dtimes.p, t.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* fp = std::fopen(c.timesPath, "wb")) {
            std::fwrite(t.data(), 8, t.size(), fp);
            std::fclose(fp);
        }
    }
    return PT_OK;
}
}  // namespace

// ================================================================== C ABI (device part)
// a radiance component (emissive materials, sky colours): finite and in [0, PT_MAX_RADIANCE]
static bool radianceOk(float v) { return std::isfinite(v) && v >= 0.0f && v <= PT_MAX_RADIANCE; }

extern "C" {

int pt_device_count(int* count) {
    if (!count) return fail(PT_ERR_INVALID, "pt_device_count: null");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return PT_OK;
}

int pt_scene_create(int device, const pt_object* objs, int64_t n, const pt_material* mats, int64_t nmat,
                    pt_scene** out) {
    if (!out || n < 0 || nmat < 0 || (n > 0 && !objs) || (nmat > 0 && !mats))
        return fail(PT_ERR_INVALID, "pt_scene_create: bad argument");
    if (n >= ((int64_t)1 << 26)) return fail(PT_ERR_INVALID, "pt_scene_create: more than 2^26 objects");
    for (int64_t i = 0; i < n; i++) {
        if (objs[i].type != PT_SPHERE && objs[i].type != PT_TRIANGLE)
            return fail(PT_ERR_INVALID, "pt_scene_create: unknown object type");
        if (objs[i].mat < 0 || objs[i].mat >= nmat) return fail(PT_ERR_INVALID, "pt_scene_create: material id out of range");
    }
    bool emissive = false;
    for (int64_t i = 0; i < nmat; i++) {   // (the other material types are taken as they come)
        if (mats[i].type != PT_EMISSIVE) continue;
        emissive = true;
        for (int a = 0; a < 3; a++)
            if (!radianceOk(mats[i].albedo[a]))
                return fail(PT_ERR_INVALID, "pt_scene_create: emissive material " + std::to_string(i) + ": radiance[" +
                                                std::to_string(a) + "] must be finite and in [0, PT_MAX_RADIANCE]");
    }
    int rc = setDevice(device);
    if (rc) return rc;
    std::unique_ptr<pt_scene> s(new pt_scene);
    s->device = device;
    s->nobj = n;
    s->nmat = nmat;
    s->hasEmissive = emissive;
    for (int64_t i = 0; i < nmat; i++)
        if (mats[i].type == PT_METAL || mats[i].type == PT_DIELECTRIC) s->lambertOnly = false;
    s->matEmissive.resize((size_t)nmat);
    for (int64_t i = 0; i < nmat; i++) s->matEmissive[(size_t)i] = mats[i].type == PT_EMISSIVE ? 1 : 0;
    s->objs.assign(objs, objs + n);
    for (int64_t i = 0; i < n && !s->hasSpheres; i++) s->hasSpheres = objs[i].type == PT_SPHERE;
    // materials: (albedo.xyz, fuzz), (ir, type, 0, 0)
    std::vector<float4> m((size_t)std::max<int64_t>(1, 2 * nmat));
    for (int64_t i = 0; i < nmat; i++) {
        m[2 * i] = make_float4(mats[i].albedo[0], mats[i].albedo[1], mats[i].albedo[2], mats[i].fuzz);
        uint32_t t = (uint32_t)mats[i].type;
        float tf;
        std::memcpy(&tf, &t, 4);
        m[2 * i + 1] = make_float4(mats[i].ir, tf, 0.0f, 0.0f);
    }
    if ((rc = devAlloc(s->mats, m.size() * sizeof(float4)))) return rc;
    HIP_TRY(hipMemcpy(s->mats.p, m.data(), m.size() * sizeof(float4), hipMemcpyHostToDevice));
    if ((rc = devAlloc(s->counters, kNumCounters * sizeof(unsigned long long)))) return rc;
    if ((rc = devAlloc(s->dobjs, (size_t)std::max<int64_t>(1, n) * sizeof(pt_object)))) return rc;
    if (n > 0) HIP_TRY(hipMemcpy(s->dobjs.p, objs, (size_t)n * sizeof(pt_object), hipMemcpyHostToDevice));
    *out = s.release();
    return PT_OK;
}

int pt_scene_set_sky(pt_scene* s, const float horizon[3], const float zenith[3]) {
    if (!s || !horizon || !zenith) return fail(PT_ERR_INVALID, "pt_scene_set_sky: null argument");
    for (int a = 0; a < 3; a++) {
        if (!radianceOk(horizon[a]))
            return fail(PT_ERR_INVALID, "pt_scene_set_sky: horizon[" + std::to_string(a) + "] must be finite and in [0, PT_MAX_RADIANCE]");
        if (!radianceOk(zenith[a]))
            return fail(PT_ERR_INVALID, "pt_scene_set_sky: zenith[" + std::to_string(a) + "] must be finite and in [0, PT_MAX_RADIANCE]");
    }
    // (host state only: the next pt_render copies it into its launch parameters)
    for (int a = 0; a < 3; a++) { s->skyH[a] = horizon[a]; s->skyZ[a] = zenith[a]; }
    return PT_OK;
}

int pt_scene_create_instanced(int device, const pt_object* objs, int64_t n, const int64_t* mesh_first,
                              const int64_t* mesh_count, int n_meshes, const pt_instance* inst, int64_t n_inst,
                              const pt_material* mats, int64_t nmat, pt_scene** out) {
    if (!out || n < 0 || n_meshes < 0 || n_inst <= 0 || (n > 0 && !objs) || (n_meshes > 0 && (!mesh_first || !mesh_count)) ||
        !inst || (nmat > 0 && !mats))
        return fail(PT_ERR_INVALID, "pt_scene_create_instanced: bad argument");
    for (int m = 0; m < n_meshes; m++)
        if (mesh_first[m] < 0 || mesh_count[m] < 0 || mesh_first[m] + mesh_count[m] > n)
            return fail(PT_ERR_INVALID, "pt_scene_create_instanced: mesh range out of bounds");
    for (int64_t i = 0; i < n_inst; i++)
        if (inst[i].mesh < 0 || inst[i].mesh >= n_meshes)
            return fail(PT_ERR_INVALID, "pt_scene_create_instanced: instance of an unknown mesh");
    pt_scene* s = nullptr;
    int rc = pt_scene_create(device, objs, n, mats, nmat, &s);
    if (rc) return rc;
    s->instanced = true;
    s->meshFirst.assign(mesh_first, mesh_first + n_meshes);
    s->meshCount.assign(mesh_count, mesh_count + n_meshes);
    s->inst.assign(inst, inst + n_inst);
    *out = s;
    return PT_OK;
}

int pt_scene_update_objects(pt_scene* s, const pt_object* objs, int64_t first, int64_t n) {
    if (!s || first < 0 || n < 0 || first > s->nobj || n > s->nobj - first || (n > 0 && !objs))
        return fail(PT_ERR_INVALID, "pt_scene_update_objects: bad argument");
    if (s->instanced) return fail(PT_ERR_INVALID, "pt_scene_update_objects: not for instanced scenes");
    for (int64_t i = 0; i < n; i++) {
        if (objs[i].type != PT_SPHERE && objs[i].type != PT_TRIANGLE)
            return fail(PT_ERR_INVALID, "pt_scene_update_objects: unknown object type");
        if (objs[i].mat < 0 || objs[i].mat >= s->nmat)
            return fail(PT_ERR_INVALID, "pt_scene_update_objects: material id out of range");
    }
    int rc = setDevice(s->device);
    if (rc) return rc;
    if (n == 0) return PT_OK;
    std::copy(objs, objs + n, s->objs.begin() + first);
    for (int64_t i = 0; i < n && !s->hasSpheres; i++) s->hasSpheres = objs[i].type == PT_SPHERE;
    HIP_TRY(hipMemcpy(s->dobjs.as<pt_object>() + first, objs, (size_t)n * sizeof(pt_object), hipMemcpyHostToDevice));
    s->built = false;   // the hierarchy no longer matches the objects: rebuild before rendering
    s->updated = true;  // from now on the wide tree is built on the device (once per rebuild)
    return PT_OK;
}

int pt_scene_update_instances(pt_scene* s, const pt_instance* inst, int64_t first, int64_t n) {
    // (the arguments that need no look at the scene first)
    if (!s || first < 0 || n < 0 || (n > 0 && !inst)) return fail(PT_ERR_INVALID, "pt_scene_update_instances: bad argument");
    if (!s->instanced) return fail(PT_ERR_INVALID, "pt_scene_update_instances: not an instanced scene");
    const int64_t ni = (int64_t)s->inst.size();
    if (first > ni || n > ni - first)
        return fail(PT_ERR_INVALID, "pt_scene_update_instances: range outside the scene's " + std::to_string(ni) + " instances");
    for (int64_t i = 0; i < n; i++) {
        const std::string who = "pt_scene_update_instances: instance " + std::to_string(first + i);
        if (inst[i].mesh != s->inst[(size_t)(first + i)].mesh)
            return fail(PT_ERR_INVALID, who + " changes its mesh (the object numbering depends on it: create a new scene)");
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(inst[i].m[k])) return fail(PT_ERR_INVALID, who + " has a non-finite matrix entry");
        std::array<float, 12> minv;
        std::array<double, 12> w2o;
        uint8_t cls;
        if (!instanceInverse(inst[i], minv, w2o, cls)) return fail(PT_ERR_INVALID, who + " has a singular transform");
    }
    if (n == 0) return PT_OK;
    std::copy(inst, inst + n, s->inst.begin() + first);
    s->built = false;        // the top level no longer matches the matrices: rebuild before rendering
    s->instDynamic = true;   // from now on builds keep the mesh trees (pt_scene_build_bvh)
    return PT_OK;
}

int pt_scene_build_bvh(pt_scene* s, int flags) { return pt_scene_build_bvh_ex(s, flags, nullptr); }

int pt_scene_build_bvh_ex(pt_scene* s, int flags, void* stream) {
    if (!s) return fail(PT_ERR_INVALID, "pt_scene_build_bvh: null scene");
    int rc = setDevice(s->device);
    if (rc) return rc;
    if (s->instanced) {   // the two-level tree (flags: the LBVH's do not apply)
        s->built = false;
        // PT_BVH_WIDE_DEVICE: lay the scene out for instance updates.  A dynamic scene's first build
        // is the full host build in that layout; later ones redo the matrix-dependent work alone,
        // unless a mesh's reach has outgrown its tree (then the full build again).
        if (flags & PT_BVH_WIDE_DEVICE) s->instDynamic = true;
        // PT_BVH_LIGHTS: the sampled lights in world space, for this build; the later builds write them
        // from the tables of a full build that had the bit.
        const bool lights = (flags & PT_BVH_LIGHTS) != 0;
        if (s->instDynamic && s->instPrepared && (!lights || s->instLightsPrepared)) {
            bool done = false;
            if ((rc = rebuildInstancedTop(s, lights, static_cast<hipStream_t>(stream), &done))) return rc;
            if (done) return PT_OK;
        }
        return buildInstanced(s, lights, static_cast<hipStream_t>(stream));
    }
    const int64_t n = s->nobj;
    s->built = false;
    s->wideReady = false;   // the wide buffers are kept for the next wide build
    s->wideSource = 0;
    s->wideNodes = 0;
    s->wideDepth = 0;
    // Everything on the device, on one stream: scene box -> Morton codes -> radix sort ->
    // leaf records -> Karras hierarchy -> refit -> depth.  (PT_BVH_HOST_KEYS: the keys come from
    // the host restatement of computeMortonOnHost instead; the result is identical.)
    const size_t n1 = (size_t)std::max<int64_t>(1, n), ni = (size_t)std::max<int64_t>(1, n - 1);
    if ((rc = devReserve(s->prims, n1 * 3 * sizeof(float4))) || (rc = devReserve(s->shade, n1 * 3 * sizeof(float4))) ||
        (rc = devReserve(s->nodes, ni * 4 * sizeof(float4))) || (rc = devReserve(s->keys, n1 * 8)) ||
        (rc = devReserve(s->leafBoxes, n1 * 24)) || (rc = devReserve(s->iparent, ni * 4)) ||
        (rc = devReserve(s->lparent, n1 * 4)) || (rc = devReserve(s->irange, ni * 8)) ||
        (rc = devReserve(s->refitEvents, (n1 + 2) * 4)))   // count + at most (crossing nodes + 1) <= n arrivals
        return rc;
    DevBuf &codes = s->codes, &ids = s->ids, &codes2 = s->codes2, &ids2 = s->ids2, &box6 = s->box6, &sph = s->sph,
           &arr = s->arr, &dep = s->dep, &temp = s->sortTemp;
    if ((rc = devReserve(codes, n1 * 4)) || (rc = devReserve(ids, n1 * 4)) || (rc = devReserve(codes2, n1 * 4)) ||
        (rc = devReserve(ids2, n1 * 4)) || (rc = devReserve(box6, (1 + kBoxBlocks) * 6 * sizeof(float))) || (rc = devReserve(sph, n1 * 4)) ||
        (rc = devReserve(arr, ni * 4)) || (rc = devReserve(dep, 16)))
        return rc;
    // The sampled lights (PT_RENDER_NEE): the host counts them to size the list (it allocates only when
    // the count or the object count grows); the list itself is the device's, on the build's stream.
    s->nLights = 0;
    uint32_t lightCap = 0;
    if (s->hasEmissive)
        for (int64_t i = 0; i < n; i++)
            lightCap += (s->objs[(size_t)i].type == PT_TRIANGLE && s->matEmissive[(size_t)s->objs[(size_t)i].mat]) ? 1u : 0u;
    if (lightCap > 0 &&
        ((rc = devReserve(s->lightFlag, n1 * 4)) || (rc = devReserve(s->lightSlot, n1 * 4)) ||
         (rc = devReserve(s->lightScan, pt::scanScratchBytesU32(n1))) ||
         (rc = devReserve(s->lights, (size_t)lightCap * 4 * sizeof(float4))) || (rc = devReserve(s->lightCount, 16))))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // Every return path destroys the events and, on failure, waits for the work already queued on
    // the stream (it uses the scene's buffers).
    StreamGuard guard(st);
    HIP_TRY(hipEventCreate(&guard.e0));
    HIP_TRY(hipEventCreate(&guard.e1));
    hipEvent_t e0 = guard.e0, e1 = guard.e1;
    HIP_TRY(hipEventRecord(e0, st));
    const unsigned tb = 256, nb = (unsigned)((n1 + tb - 1) / tb), nbi = (unsigned)((ni + tb - 1) / tb);
    if (n > 0) {
        if (flags & PT_BVH_HOST_KEYS) {
            std::vector<uint64_t> hk((size_t)n);
            pt::mortonKeys(s->objs.data(), n, (flags & PT_BVH_ORIGIN_BOUNDS) != 0, hk.data());
            std::vector<uint32_t> hc((size_t)n), hi((size_t)n);
            for (int64_t k = 0; k < n; k++) { hc[k] = (uint32_t)(hk[k] >> 32); hi[k] = (uint32_t)hk[k]; }
            HIP_TRY(hipMemcpyAsync(codes2.p, hc.data(), n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ids2.p, hi.data(), n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        } else {
            const int inc = (flags & PT_BVH_ORIGIN_BOUNDS) ? 1 : 0;
            sceneBoxKernel<<<kBoxBlocks, 1024, 0, st>>>(s->dobjs.as<pt_object>(), n, inc, box6.as<float>(),
                                                        box6.as<float>() + 6);
            sceneBoxKernel<<<1, 1024, 0, st>>>(s->dobjs.as<pt_object>(), n, inc, box6.as<float>(), nullptr);
            mortonKernel<<<nb, tb, 0, st>>>(s->dobjs.as<pt_object>(), n, box6.as<float>(), codes.as<uint32_t>(),
                                            ids.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            if ((rc = sortPairs(temp, codes.as<uint32_t>(), codes2.as<uint32_t>(), ids.as<uint32_t>(), ids2.as<uint32_t>(),
                                (size_t)n, 30, st)))
                return rc;
        }
        leafGatherKernel<<<nb, tb, 0, st>>>(s->dobjs.as<pt_object>(), codes2.as<uint32_t>(), ids2.as<uint32_t>(), n,
                                            s->keys.as<unsigned long long>(), s->prims.as<float4>(),
                                            s->shade.as<float4>(), s->leafBoxes.as<float>(), sph.as<uint32_t>(),
                                            s->mats.as<float4>());
        HIP_TRY(hipGetLastError());
        if (lightCap > 0) {
            lightFlagKernel<<<nb, tb, 0, st>>>(s->dobjs.as<pt_object>(), n, s->mats.as<float4>(), s->lightFlag.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(pt::exclusiveScanU32(s->lightScan.p, s->lightFlag.as<uint32_t>(), s->lightSlot.as<uint32_t>(), (size_t)n, st));
            lightListKernel<<<nb, tb, 0, st>>>(s->dobjs.as<pt_object>(), n, s->mats.as<float4>(), s->lightFlag.as<uint32_t>(),
                                               s->lightSlot.as<uint32_t>(), lightCap, s->lights.as<float4>(),
                                               s->lightCount.as<uint32_t>());
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipMemsetAsync(s->nodes.p, 0, ni * 4 * sizeof(float4), st));
    HIP_TRY(hipMemsetAsync(s->iparent.p, 0xff, ni * 4, st));
    HIP_TRY(hipMemsetAsync(s->lparent.p, 0xff, n1 * 4, st));
    HIP_TRY(hipMemsetAsync(arr.p, 0, ni * 4, st));
    HIP_TRY(hipMemsetAsync(s->refitEvents.p, 0, 4, st));
    HIP_TRY(hipMemsetAsync(dep.p, 0, 16, st));
    if (n > 1) {
        karrasKernel<<<nbi, tb, 0, st>>>(s->keys.as<unsigned long long>(), (int)n, s->nodes.as<float4>(),
                                         s->iparent.as<int>(), s->lparent.as<int>(), sph.as<uint32_t>(),
                                         s->irange.as<int2>());
        HIP_TRY(hipGetLastError());
        refitKernel<<<(unsigned)((n + kRefitBlock - 1) / kRefitBlock), kRefitBlock, 0, st>>>(
            s->nodes.as<float4>(), s->iparent.as<int>(), s->lparent.as<int>(), s->irange.as<int2>(),
            s->leafBoxes.as<float>(), s->refitEvents.as<unsigned int>(), (int)n);
        refitTopKernel<<<1, kRefitTop, 0, st>>>(s->nodes.as<float4>(), s->iparent.as<int>(),
                                                s->refitEvents.as<unsigned int>(), arr.as<unsigned int>());
        HIP_TRY(hipGetLastError());
        depthKernel<<<nb, tb, 0, st>>>(s->iparent.as<int>(), s->lparent.as<int>(), (int)n, dep.as<int>());
        HIP_TRY(hipGetLastError());
    }
    if ((flags & PT_BVH_WIDE_DEVICE) && n > 0) {
        if ((rc = buildWideDevice(s, st))) return rc;
        s->wideReady = true;
        s->wideBuildMs = 0.0;
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    guard.ok = true;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    s->buildMs = ms;
    int depth = 0;
    HIP_TRY(hipMemcpy(&depth, dep.p, 4, hipMemcpyDeviceToHost));
    s->depth = n > 1 ? depth : 0;
    if (lightCap > 0) {
        uint32_t nl = 0;
        HIP_TRY(hipMemcpy(&nl, s->lightCount.p, 4, hipMemcpyDeviceToHost));
        if (nl != lightCap) return fail(PT_ERR_STATE, "pt_scene_build_bvh: the device's light list disagrees with the host's count");
        s->nLights = (int64_t)nl;
    }
    if (n > 0) {   // the tight scene box: union of the root's child boxes (a single object: its box)
        float mn[3], mx[3];
        if (n > 1) {
            float r[12];
            HIP_TRY(hipMemcpy(r, s->nodes.p, sizeof(r), hipMemcpyDeviceToHost));
            for (int a = 0; a < 3; a++) {
                mn[a] = std::fmin(r[nodeBoxIdx(0, a, 0)], r[nodeBoxIdx(1, a, 0)]);
                mx[a] = std::fmax(r[nodeBoxIdx(0, a, 1)], r[nodeBoxIdx(1, a, 1)]);
            }
        } else {
            float b6[6];
            HIP_TRY(hipMemcpy(b6, s->leafBoxes.p, sizeof(b6), hipMemcpyDeviceToHost));
            for (int a = 0; a < 3; a++) { mn[a] = b6[a]; mx[a] = b6[3 + a]; }
        }
        float e = 0.0f;
        double m = 0.0;
        for (int a = 0; a < 3; a++) {
            s->sceneCE[a] = 0.5f * (mn[a] + mx[a]);
            e = std::fmax(e, mx[a] - mn[a]);
            m = std::max({m, std::fabs((double)mn[a]), std::fabs((double)mx[a]), (double)mx[a] - (double)mn[a]});
        }
        s->sceneCE[3] = e;
        s->mixLim = mixLimit(m);
    }
    if (n > 1 && stackFor(s->depth) < 0) return fail(PT_ERR_STATE, "BVH too deep");
    if (s->wideReady && wideStackFor(s->wideDepth) < 0) return fail(PT_ERR_STATE, "wide BVH too deep");
    s->deviceBytes = (size_t)(n > 1 ? n - 1 : 0) * 64 + (size_t)n * 96 + (size_t)s->nmat * 32;
    s->built = true;
    return PT_OK;
}

// The wide tree is only needed by PT_KERNEL_WIDE: unless pt_scene_build_bvh built it on the
// device (PT_BVH_WIDE_DEVICE), built on first use after each LBVH build -- on the device for a
// scene whose objects were updated (dynamic: a rebuild per frame) or when PT_WIDE_BUILD=device,
// else on the host (binned SAH: a few percent faster to trace, slower to build).
static int ensureWide(pt_scene* s) {
    if (s->wideReady || s->nobj <= 0) return PT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const char* wb = std::getenv("PT_WIDE_BUILD");
    const std::string wbs = wb ? wb : "";
    const bool device = wbs == "device" || (s->updated && wbs != "host");
    int rc = device ? buildWideDevice(s, 0) : buildWide(s);
    if (!rc && s->wideSource == 2) HIP_TRY(hipStreamSynchronize(0));
    if (rc) return rc;
    s->wideReady = true;
    s->wideBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (wideStackFor(s->wideDepth) < 0) return fail(PT_ERR_STATE, "wide BVH too deep");
    return PT_OK;
}

int pt_scene_wide_info(pt_scene* s, int* depth, int64_t* slots, double* ms, int* source) {
    if (!s) return fail(PT_ERR_INVALID, "pt_scene_wide_info: null scene");
    const bool ok = s->wideReady;
    if (depth) *depth = ok ? s->wideDepth : 0;
    if (slots) *slots = ok ? s->wideNodes : 0;
    if (ms) *ms = ok ? s->wideBuildMs : 0.0;
    if (source) *source = ok ? s->wideSource : 0;
    return PT_OK;
}

int pt_scene_light_count(pt_scene* s, int64_t* n) {
    if (!s || !n) return fail(PT_ERR_INVALID, "pt_scene_light_count: null argument");
    if (!s->built) return fail(PT_ERR_STATE, "pt_scene_light_count: BVH not built");
    *n = s->nLights;
    return PT_OK;
}

int pt_scene_download_lights(pt_scene* s, float* records) {
    if (!s) return fail(PT_ERR_INVALID, "pt_scene_download_lights: null scene");
    if (!s->built) return fail(PT_ERR_STATE, "pt_scene_download_lights: BVH not built");
    const int64_t n = s->nLights;
    if (n == 0) return PT_OK;
    if (!records) return fail(PT_ERR_INVALID, "pt_scene_download_lights: null records");
    int rc = setDevice(s->device);
    if (rc) return rc;
    std::vector<float> rec((size_t)n * 16);
    HIP_TRY(hipMemcpy(rec.data(), s->lights.p, rec.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++)
        for (int v = 0; v < 4; v++) std::memcpy(records + 12 * i + 3 * v, &rec[(size_t)(16 * i + 4 * v)], 12);
    return PT_OK;
}

int pt_scene_build_time(pt_scene* s, double* ms) {
    if (!s || !ms) return fail(PT_ERR_INVALID, "pt_scene_build_time: null argument");
    if (!s->built) return fail(PT_ERR_STATE, "BVH not built");
    *ms = s->buildMs;
    return PT_OK;
}

int pt_scene_bvh_info(pt_scene* s, int* depth, int64_t* nodes, int64_t* bytes) {
    if (!s) return fail(PT_ERR_INVALID, "pt_scene_bvh_info: null scene");
    if (!s->built) return fail(PT_ERR_STATE, "BVH not built");
    if (depth) *depth = s->depth;
    if (nodes) *nodes = s->nobj > 0 ? 2 * s->nobj - 1 : 0;
    // (+ the wide kernels' exact-box array once the wide tree exists; like the wide tree's nodes and
    // its primitive records, the edge-form records of a triangle-only scene are not in this count)
    if (bytes) *bytes = (int64_t)(s->deviceBytes + (s->wideReady && !s->instanced ? (size_t)s->nobj * pt::kW8BoxFloats * 4 : 0));
    return PT_OK;
}

int pt_scene_download_bvh(pt_scene* s, pt_bvh_node* out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "pt_scene_download_bvh: null argument");
    if (!s->built) return fail(PT_ERR_STATE, "BVH not built");
    if (s->instanced) return fail(PT_ERR_STATE, "pt_scene_download_bvh: an instanced scene has no LBVH");
    int rc = setDevice(s->device);
    if (rc) return rc;
    const int64_t n = s->nobj;
    if (n <= 0) return PT_OK;
    const int64_t L = n - 1;
    std::vector<float4> nodes((size_t)std::max<int64_t>(1, L) * 4);
    std::vector<uint64_t> keys((size_t)n);
    std::vector<int32_t> iparent((size_t)std::max<int64_t>(1, L)), lparent((size_t)n);
    std::vector<float> leafBoxes((size_t)n * 6);
    if (L > 0) HIP_TRY(hipMemcpy(nodes.data(), s->nodes.p, L * 4 * sizeof(float4), hipMemcpyDeviceToHost));
    if (L > 0) HIP_TRY(hipMemcpy(iparent.data(), s->iparent.p, L * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys.data(), s->keys.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lparent.data(), s->lparent.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(leafBoxes.data(), s->leafBoxes.p, n * 24, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < 2 * n - 1; i++) {
        out[i].left = out[i].right = out[i].parent = out[i].objid = -1;
        for (int a = 0; a < 3; a++) out[i].bmin[a] = out[i].bmax[a] = 0.0f;
    }
    auto refIndex = [&](uint32_t r) -> int64_t { return (r & kLeafBit) ? L + (int64_t)(r & kPrimMask) : (int64_t)r; };
    for (int64_t k = 0; k < n; k++) {
        out[L + k].objid = (int32_t)(keys[k] & 0xffffffffu);
        out[L + k].parent = L > 0 ? lparent[k] : -1;
    }
    for (int64_t i = 0; i < L; i++) {
        const float* f = reinterpret_cast<const float*>(&nodes[4 * i]);
        uint32_t lr, rr;
        std::memcpy(&lr, f + 12, 4);
        std::memcpy(&rr, f + 13, 4);
        out[i].left = (int32_t)refIndex(lr);
        out[i].right = (int32_t)refIndex(rr);
        out[i].parent = i == 0 ? -1 : iparent[i];
        for (int c = 0; c < 2; c++) {   // child boxes live in this record; copy them to the child
            pt_bvh_node& ch = out[c == 0 ? out[i].left : out[i].right];
            for (int a = 0; a < 3; a++) { ch.bmin[a] = f[nodeBoxIdx(c, a, 0)]; ch.bmax[a] = f[nodeBoxIdx(c, a, 1)]; }
        }
        if (i == 0) {   // the root's own box (never tested by the traversal)
            for (int a = 0; a < 3; a++) {
                out[0].bmin[a] = std::fmin(f[nodeBoxIdx(0, a, 0)], f[nodeBoxIdx(1, a, 0)]);
                out[0].bmax[a] = std::fmax(f[nodeBoxIdx(0, a, 1)], f[nodeBoxIdx(1, a, 1)]);
            }
        }
    }
    if (L == 0) {   // single object: the root is the leaf (bvh.h:76-81 with numObjects = 1)
        for (int a = 0; a < 3; a++) { out[0].bmin[a] = leafBoxes[a]; out[0].bmax[a] = leafBoxes[3 + a]; }
    }
    return PT_OK;
}

int pt_scene_download_wide(pt_scene* s, int array, void* out, int64_t capacity, int64_t* bytes) {
    if (bytes) *bytes = 0;
    if (!s) return fail(PT_ERR_INVALID, "pt_scene_download_wide: null scene");
    if (array < PT_WIDE_NODES || array > PT_WIDE_INSTANCES) return fail(PT_ERR_INVALID, "pt_scene_download_wide: unknown array");
    if (capacity < 0) return fail(PT_ERR_INVALID, "pt_scene_download_wide: negative capacity");
    if (!s->built) return fail(PT_ERR_STATE, "pt_scene_download_wide: BVH not built");
    int rc = setDevice(s->device);
    if (rc) return rc;
    if ((rc = ensureWide(s))) return rc;   // (first use: builds the tree, as a query does)
    // the arrays as the kernels read them (devScene): a flat scene's are sized by its objects, an
    // instanced scene's by its full build
    const size_t n = s->wideReady && !s->instanced ? (size_t)s->nobj : 0;
    const DevBuf* src = nullptr;
    size_t size = 0;
    switch (array) {
    case PT_WIDE_NODES: src = &s->wide; size = s->wideReady ? (size_t)s->wideNodes * pt::kW8NodeDwords * 4 : 0; break;
    case PT_WIDE_PRIMS: src = &s->wprims; size = s->instanced ? s->instPrimBytes : n * pt::kW8PrimDwords * 4; break;
    case PT_WIDE_SHADE: src = &s->wshade; size = s->instanced ? s->instShadeBytes : n * 48; break;
    case PT_WIDE_BOXES: src = &s->wbox; size = n * pt::kW8BoxFloats * 4; break;
    case PT_WIDE_RANKS: src = &s->rankOf; size = n * 4; break;
    case PT_WIDE_EDGE_PRIMS: src = &s->wtris; size = s->haveWtris ? n * pt::kW8PrimDwords * 4 : 0; break;
    default: src = &s->winst; size = s->instanced ? s->instWinstBytes : 0; break;
    }
    if (size > 0 && (!src->p || src->cap < size)) return fail(PT_ERR_STATE, "pt_scene_download_wide: the array is smaller than the tree reports");
    if (bytes) *bytes = (int64_t)size;
    if (!out || size == 0) return PT_OK;
    if ((uint64_t)capacity < size) return fail(PT_ERR_INVALID, "pt_scene_download_wide: capacity below the array's size");
    HIP_TRY(hipDeviceSynchronize());   // (a build has finished when it returns; renders only read the arrays)
    HIP_TRY(hipMemcpy(out, src->p, size, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"

namespace {
// The ray queries' interval contract (include/pt.h, pt_trace_closest): tmin >= 0 and not NaN (-0.0
// counts as 0), the scalar tmax not NaN; tmax < tmin is a legal, empty interval.  Checked by every
// entry point before anything is allocated or launched.  (The kernels' accept tests rely on it:
// `t >= 0.0f` with -1 as the miss marker.)
int checkInterval(const char* who, float tmin, float tmax, bool scalarTmax = true) {
    if (!(tmin >= 0.0f)) return fail(PT_ERR_INVALID, std::string(who) + ": tmin must be >= 0 and not NaN");
    if (scalarTmax && std::isnan(tmax)) return fail(PT_ERR_INVALID, std::string(who) + ": tmax must not be NaN");
    return PT_OK;
}
// A batch of n ray queries on device arrays, traced on `st`; the host waits for the end (counters
// and the guard word are read back).  `who` prefixes the messages; defaultWide: PT_KERNEL_DEFAULT
// is the wide tree (closest hit: for instanced scenes only; occlusion: always, the answer has no
// order to honour); launch(stack, wide, scene, counters) is dispatchTrace or dispatchOccluded.
template <class Launch>
int queryDevice(pt_scene* s, const char* who, int kernel, bool defaultWide, int64_t n, hipStream_t st, pt_stats* stats,
                Launch launch) {
    if (kernel != PT_KERNEL_DEFAULT && kernel != PT_KERNEL_SIMPLE && kernel != PT_KERNEL_WAVEFRONT &&
        kernel != PT_KERNEL_WIDE)
        return fail(PT_ERR_INVALID, std::string(who) + ": unknown kernel");
    if (!s->built) return fail(PT_ERR_STATE, "BVH not built");
    int rc = setDevice(s->device);
    if (rc) return rc;
    const bool wide = kernel == PT_KERNEL_WIDE || (kernel == PT_KERNEL_DEFAULT && defaultWide);
    if (s->instanced && !wide)
        return fail(PT_ERR_INVALID, std::string(who) + ": instanced scenes trace with the wide kernel");
    if (wide && (rc = ensureWide(s))) return rc;
    const int stack = wide ? wideStackFor(s->wideDepth) : (s->nobj > 1 ? stackFor(s->depth) : 16);
    StreamGuard guard(st);
    HIP_TRY(hipMemsetAsync(s->counters.p, 0, kNumCounters * sizeof(unsigned long long), st));
    HIP_TRY(hipEventCreate(&guard.e0));
    HIP_TRY(hipEventCreate(&guard.e1));
    HIP_TRY(hipEventRecord(guard.e0, st));
    if (n > 0 && (rc = launch(stack, wide, devScene(s), s->counters.as<unsigned long long>()))) return rc;
    HIP_TRY(hipEventRecord(guard.e1, st));
    HIP_TRY(hipEventSynchronize(guard.e1));
    guard.ok = true;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, guard.e0, guard.e1));
    unsigned long long c[kNumCounters] = {0};
    HIP_TRY(hipMemcpy(c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    c[4] = 0;
    fillStats(stats, c, ms, wide);
    if (c[7]) return fail(PT_ERR_STATE, "traversal guard tripped (corrupt BVH), flags " + std::to_string(c[7]));
    return PT_OK;
}
// Closest hits / occlusion flags of n rays: dr, dh / drt, docc are device arrays.
int traceDevice(pt_scene* s, const pt_ray* dr, int64_t n, float tmin, float tmax, int kernel, pt_hit* dh,
                hipStream_t st, pt_stats* stats) {
    return queryDevice(s, "pt_trace_closest", kernel, s->instanced, n, st, stats,
                       [&](int stack, bool wide, const DevScene& S, unsigned long long* cnt) {
                           return dispatchTrace(stack, wide, S, dr, n, tmin, tmax, dh, cnt, st);
                       });
}
int occludedDevice(pt_scene* s, const pt_ray* dr, int64_t n, float tmin, float tmax, const float* drt, int kernel,
                   uint8_t* docc, hipStream_t st, pt_stats* stats) {
    return queryDevice(s, "pt_trace_occluded", kernel, true, n, st, stats,
                       [&](int stack, bool wide, const DevScene& S, unsigned long long* cnt) {
                           return dispatchOccluded(stack, wide, S, dr, n, tmin, tmax, drt, docc, cnt, st);
                       });
}
}  // namespace

extern "C" {

int pt_trace_closest(pt_scene* s, const pt_ray* rays, int64_t n, float tmin, float tmax, pt_hit* hits,
                     pt_stats* stats) {
    if (int rc = checkInterval("pt_trace_closest", tmin, tmax)) return rc;
    return pt_trace_closest_ex(s, rays, n, tmin, tmax, PT_KERNEL_DEFAULT, hits, stats);
}

int pt_trace_closest_ex(pt_scene* s, const pt_ray* rays, int64_t n, float tmin, float tmax, int kernel, pt_hit* hits,
                        pt_stats* stats) {
    if (!s || n < 0 || (n > 0 && (!rays || !hits))) return fail(PT_ERR_INVALID, "pt_trace_closest: bad argument");
    int rc = checkInterval("pt_trace_closest_ex", tmin, tmax);
    if (rc || (rc = setDevice(s->device))) return rc;
    DevBuf dr, dh;
    if ((rc = devAlloc(dr, n * sizeof(pt_ray))) || (rc = devAlloc(dh, n * sizeof(pt_hit)))) return rc;
    if (n > 0) HIP_TRY(hipMemcpy(dr.p, rays, n * sizeof(pt_ray), hipMemcpyHostToDevice));
    if ((rc = traceDevice(s, dr.as<pt_ray>(), n, tmin, tmax, kernel, dh.as<pt_hit>(), 0, stats))) return rc;
    if (n > 0) HIP_TRY(hipMemcpy(hits, dh.p, n * sizeof(pt_hit), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_trace_closest_device(pt_scene* s, const pt_ray* rays, int64_t n, float tmin, float tmax, int kernel,
                            pt_hit* hits, void* stream, pt_stats* stats) {
    if (!s || n < 0 || (n > 0 && (!rays || !hits))) return fail(PT_ERR_INVALID, "pt_trace_closest_device: bad argument");
    if (int rc = checkInterval("pt_trace_closest_device", tmin, tmax)) return rc;
    return traceDevice(s, rays, n, tmin, tmax, kernel, hits, static_cast<hipStream_t>(stream), stats);
}

int pt_trace_occluded(pt_scene* s, const pt_ray* rays, int64_t n, float tmin, float tmax, const float* ray_tmax,
                      int kernel, uint8_t* occluded, pt_stats* stats) {
    if (!s || n < 0 || (n > 0 && (!rays || !occluded))) return fail(PT_ERR_INVALID, "pt_trace_occluded: bad argument");
    int rc = checkInterval("pt_trace_occluded", tmin, tmax, !ray_tmax);
    if (rc || (rc = setDevice(s->device))) return rc;
    DevBuf dr, dt, dq;
    if ((rc = devAlloc(dr, n * sizeof(pt_ray))) || (rc = devAlloc(dq, n))) return rc;
    if (ray_tmax && (rc = devAlloc(dt, n * sizeof(float)))) return rc;
    if (n > 0) HIP_TRY(hipMemcpy(dr.p, rays, n * sizeof(pt_ray), hipMemcpyHostToDevice));
    if (n > 0 && ray_tmax) HIP_TRY(hipMemcpy(dt.p, ray_tmax, n * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = occludedDevice(s, dr.as<pt_ray>(), n, tmin, tmax, n > 0 && ray_tmax ? dt.as<float>() : nullptr, kernel,
                             dq.as<uint8_t>(), 0, stats)))
        return rc;
    if (n > 0) HIP_TRY(hipMemcpy(occluded, dq.p, n, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_trace_occluded_device(pt_scene* s, const pt_ray* rays, int64_t n, float tmin, float tmax, const float* ray_tmax,
                             int kernel, uint8_t* occluded, void* stream, pt_stats* stats) {
    if (!s || n < 0 || (n > 0 && (!rays || !occluded)))
        return fail(PT_ERR_INVALID, "pt_trace_occluded_device: bad argument");
    if (int rc = checkInterval("pt_trace_occluded_device", tmin, tmax, !ray_tmax)) return rc;
    return occludedDevice(s, rays, n, tmin, tmax, ray_tmax, kernel, occluded, static_cast<hipStream_t>(stream), stats);
}

int pt_film_create(int device, int width, int height, int sh, int nparts, int part, uint64_t seed, pt_film** out) {
    if (!out || width <= 0 || height <= 0 || sh <= 0 || nparts <= 0 || part < 0 || part >= nparts)
        return fail(PT_ERR_INVALID, "pt_film_create: bad argument");
    if ((int64_t)width * height >= (1ll << kJumpMats)) return fail(PT_ERR_INVALID, "pt_film_create: frame too large");
    int rc = setDevice(device);
    if (rc) return rc;
    std::unique_ptr<pt_film> f(new pt_film);
    f->device = device;
    f->width = width;
    f->height = height;
    f->stripe_h = sh;
    f->nparts = nparts;
    f->part = part;
    int rows = 0;
    for (int r = 0; r < height; r++)
        if ((r / sh) % nparts == part) rows++;
    f->nrows = rows;
    f->npix = (int64_t)rows * width;
    if ((rc = devAlloc(f->state, (size_t)std::max<int64_t>(1, f->npix) * 6 * 4))) return rc;
    f->seed = seed;
    const std::vector<uint32_t>& jm = jumpMatrices();
    if ((rc = devAlloc(f->jumps, jm.size() * 4))) return rc;
    HIP_TRY(hipMemcpy(f->jumps.p, jm.data(), jm.size() * 4, hipMemcpyHostToDevice));
    if ((rc = filmInit(f.get(), 0))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = f.release();
    return PT_OK;
}

int pt_film_reset(pt_film* f, void* stream) {
    if (!f) return fail(PT_ERR_INVALID, "pt_film_reset: null film");
    int rc = setDevice(f->device);
    if (rc) return rc;
    return filmInit(f, (hipStream_t)stream);
}

int pt_film_clear(pt_film* f, void* stream) {
    if (!f) return fail(PT_ERR_INVALID, "pt_film_clear: null film");
    int rc = setDevice(f->device);
    if (rc) return rc;
    if (f->accum.p) HIP_TRY(hipMemsetAsync(f->accum.p, 0, (size_t)std::max<int64_t>(1, f->npix) * 12, (hipStream_t)stream));
    f->accumSamples = 0;
    return PT_OK;
}

int pt_film_accumulated(pt_film* f, int64_t* samples) {
    if (!f || !samples) return fail(PT_ERR_INVALID, "pt_film_accumulated: null argument");
    *samples = f->accumSamples;
    return PT_OK;
}

int pt_film_info(pt_film* f, int* nrows, int64_t* npix) {
    if (!f) return fail(PT_ERR_INVALID, "pt_film_info: null film");
    if (nrows) *nrows = f->nrows;
    if (npix) *npix = f->npix;
    return PT_OK;
}

int pt_film_rows(pt_film* f, int32_t* rows) {
    if (!f || !rows) return fail(PT_ERR_INVALID, "pt_film_rows: null argument");
    int k = 0;
    for (int r = 0; r < f->height; r++)
        if ((r / f->stripe_h) % f->nparts == f->part) rows[k++] = r;
    return PT_OK;
}

int pt_film_get_rng(pt_film* f, uint32_t* states) {
    if (!f || !states) return fail(PT_ERR_INVALID, "pt_film_get_rng: null argument");
    int rc = setDevice(f->device);
    if (rc) return rc;
    const int64_t np = f->npix;
    std::vector<uint32_t> soa((size_t)np * 6);
    if (np) HIP_TRY(hipMemcpy(soa.data(), f->state.p, np * 24, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < np; i++)
        for (int w = 0; w < 6; w++) states[6 * i + w] = soa[(size_t)w * np + i];
    return PT_OK;
}

int pt_film_set_rng(pt_film* f, const uint32_t* states) {
    if (!f || !states) return fail(PT_ERR_INVALID, "pt_film_set_rng: null argument");
    int rc = setDevice(f->device);
    if (rc) return rc;
    const int64_t np = f->npix;
    std::vector<uint32_t> soa((size_t)np * 6);
    for (int64_t i = 0; i < np; i++)
        for (int w = 0; w < 6; w++) soa[(size_t)w * np + i] = states[6 * i + w];
    if (np) HIP_TRY(hipMemcpy(f->state.p, soa.data(), np * 24, hipMemcpyHostToDevice));
    return PT_OK;
}

int pt_render_aov(pt_scene* s, pt_film* f, const pt_camera* cam, pt_aov* out, int on_dev, void* stream,
                  pt_stats* stats) {
    static_assert(sizeof(pt_aov) == 48, "pt_aov: three 16-byte rows");
    if (!s || !f || !cam || !out) return fail(PT_ERR_INVALID, "pt_render_aov: null argument");
    if (!s->built) return fail(PT_ERR_STATE, "pt_render_aov: BVH not built");
    if (s->device != f->device) return fail(PT_ERR_INVALID, "pt_render_aov: scene and film on different devices");
    int rc = setDevice(s->device);
    if (rc || (rc = ensureWide(s))) return rc;   // (first use: builds the tree)
    hipStream_t st = on_dev ? (hipStream_t)stream : 0;
    const int64_t np = f->npix;
    void* dst = out;
    if (!on_dev) {
        if ((rc = devReserve(f->aovStaging, (size_t)std::max<int64_t>(1, np) * sizeof(pt_aov)))) return rc;
        dst = f->aovStaging.p;
    }
    AovCam c;
    for (int a = 0; a < 3; a++) {
        c.pos[a] = cam->origin[a];
        c.ll[a] = cam->lower_left[a];
        c.hor[a] = cam->horizontal[a];
        c.ver[a] = cam->vertical[a];
    }
    c.invW = 1.0f / (float)f->width;
    c.invH = 1.0f / (float)f->height;
    c.width = f->width;
    c.stripe_h = f->stripe_h;
    c.nparts = f->nparts;
    c.part = f->part;
    const bool wait = !on_dev || stats;
    const int stack = wideStackFor(s->wideDepth);
    unsigned long long* cnt = s->counters.as<unsigned long long>();
    StreamGuard guard(st);
    HIP_TRY(hipMemsetAsync(cnt, 0, kNumCounters * sizeof(unsigned long long), st));
    if (wait) {
        HIP_TRY(hipEventCreate(&guard.e0));
        HIP_TRY(hipEventCreate(&guard.e1));
        HIP_TRY(hipEventRecord(guard.e0, st));
    }
    if (np > 0 && (rc = dispatchAov(stack, devScene(s), c, np, static_cast<float4*>(dst), cnt, st))) return rc;
    if (!wait) {   // enqueued: nothing is read back (a synchronous call reports a tripped traversal guard)
        guard.ok = true;
        return PT_OK;
    }
    HIP_TRY(hipEventRecord(guard.e1, st));
    HIP_TRY(hipEventSynchronize(guard.e1));
    guard.ok = true;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, guard.e0, guard.e1));
    unsigned long long k[kNumCounters] = {0};
    HIP_TRY(hipMemcpy(k, cnt, sizeof(k), hipMemcpyDeviceToHost));
    k[4] = 0;
    fillStats(stats, k, ms, true);
    if (k[7]) return fail(PT_ERR_STATE, "traversal guard tripped (corrupt BVH), flags " + std::to_string(k[7]));
    if (!on_dev && np > 0) HIP_TRY(hipMemcpy(out, dst, (size_t)np * sizeof(pt_aov), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_film_denoise(pt_film* f, const float* rgb, const pt_aov* aov, float* out, int on_dev, void* stream,
                    const pt_denoise_opts* opts) {
    const pt_denoise_opts dflt = {5, 0.6f, 0.1f, 0.02f, {0, 0, 0, 0}};
    const pt_denoise_opts o = opts ? *opts : dflt;
    if (o.iterations < 0 || o.iterations > 8) return fail(PT_ERR_INVALID, "pt_film_denoise: iterations must lie in [0, 8]");
    for (const float sg : {o.sigma_color, o.sigma_albedo, o.sigma_plane})
        if (!std::isfinite(sg) || !(sg > 0.0f)) return fail(PT_ERR_INVALID, "pt_film_denoise: every sigma must be finite and > 0");
    if (!f || !rgb || !aov || !out) return fail(PT_ERR_INVALID, "pt_film_denoise: null argument");
    if (f->nparts != 1) return fail(PT_ERR_INVALID, "pt_film_denoise: the film must own the whole frame (n_parts == 1)");
    int rc = setDevice(f->device);
    if (rc) return rc;
    hipStream_t st = on_dev ? (hipStream_t)stream : 0;
    const size_t bytes = (size_t)f->npix * 12;
    const int n = o.iterations;
    if (n > 1 && (rc = devReserve(f->dnA, bytes))) return rc;
    if (n > 2 && (rc = devReserve(f->dnB, bytes))) return rc;
    const float* src = rgb;
    float* dst = out;
    if (!on_dev) {
        if ((rc = devReserve(f->dnRgb, bytes)) || (rc = devReserve(f->dnAov, (size_t)f->npix * sizeof(pt_aov)))) return rc;
        HIP_TRY(hipMemcpyAsync(f->dnRgb.p, rgb, bytes, hipMemcpyHostToDevice, st));
        if (n > 0) HIP_TRY(hipMemcpyAsync(f->dnAov.p, aov, (size_t)f->npix * sizeof(pt_aov), hipMemcpyHostToDevice, st));
        src = dst = f->dnRgb.as<float>();
        aov = f->dnAov.as<pt_aov>();
    }
    StreamWait guard(st);
    // Pass i reads the previous pass's image and writes a scratch image, A and B in turn; the last pass
    // writes `dst` -- through A when it would read `dst` itself (one pass, out == rgb).
    if (n == 0 && dst != src) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    if (n == 1 && dst == src && (rc = devReserve(f->dnA, bytes))) return rc;
    const float isa2 = 1.0f / (o.sigma_albedo * o.sigma_albedo);
    const float* cur = src;
    for (int i = 0; i < n; i++) {
        const float sc = o.sigma_color * (1.0f / (float)(1 << i));   // (exact: a power of two)
        const float isc2 = 1.0f / (sc * sc);
        const bool last = i == n - 1;
        float* to = last && cur != dst ? dst : (i & 1) ? f->dnB.as<float>() : f->dnA.as<float>();
        HIP_TRY(pt::atrousPass(cur, aov, to, f->width, f->height, 1 << i, isa2, isc2, o.sigma_plane, st));
        if (last && to != dst) HIP_TRY(hipMemcpyAsync(dst, to, bytes, hipMemcpyDeviceToDevice, st));
        cur = to;
    }
    if (!on_dev) {
        HIP_TRY(hipMemcpyAsync(out, f->dnRgb.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    guard.ok = true;
    return PT_OK;
}

int pt_film_temporal(pt_film* f, const float* rgb, const pt_aov* aov, const pt_camera* cam, float* out, float* out_len,
                     int on_dev, void* stream, const pt_temporal_opts* opts) {
    static_assert(sizeof(pt_temporal_opts) == 32, "pt_temporal_opts: eight 4-byte fields");
    const pt_temporal_opts dflt = {32.0f, 0.02f, 0.9f, 0, {0, 0, 0, 0}};
    const pt_temporal_opts o = opts ? *opts : dflt;
    if (!std::isfinite(o.max_history) || !(o.max_history >= 1.0f))
        return fail(PT_ERR_INVALID, "pt_film_temporal: max_history must be finite and >= 1");
    if (!std::isfinite(o.sigma_plane) || !(o.sigma_plane > 0.0f))
        return fail(PT_ERR_INVALID, "pt_film_temporal: sigma_plane must be finite and > 0");
    if (!(o.normal_cos >= -1.0f && o.normal_cos <= 1.0f))
        return fail(PT_ERR_INVALID, "pt_film_temporal: normal_cos must lie in [-1, 1]");
    if (!f || !rgb || !aov || !cam || !out) return fail(PT_ERR_INVALID, "pt_film_temporal: null argument");
    if (f->nparts != 1) return fail(PT_ERR_INVALID, "pt_film_temporal: the film must own the whole frame (n_parts == 1)");
    int rc = setDevice(f->device);
    if (rc) return rc;
    hipStream_t st = on_dev ? (hipStream_t)stream : 0;
    const size_t np = (size_t)f->npix;
    for (DevBuf& h : f->tpHist)
        if ((rc = devReserve(h, np * pt::kHistoryBytes))) return rc;
    const float* src = rgb;
    float *dst = out, *dlen = out_len;
    if (!on_dev) {
        if ((rc = devReserve(f->tpRgb, np * 12)) || (rc = devReserve(f->tpAov, np * sizeof(pt_aov)))) return rc;
        if (out_len && (rc = devReserve(f->tpLen, np * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(f->tpRgb.p, rgb, np * 12, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(f->tpAov.p, aov, np * sizeof(pt_aov), hipMemcpyHostToDevice, st));
        src = dst = f->tpRgb.as<float>();
        aov = f->tpAov.as<pt_aov>();
        dlen = out_len ? f->tpLen.as<float>() : nullptr;
    }
    StreamWait guard(st);
    pt::TemporalParams K;
    for (int a = 0; a < 3; a++) {
        K.o[a] = f->tpCam.origin[a];
        K.ll[a] = f->tpCam.lower_left[a];
        K.hor[a] = f->tpCam.horizontal[a];
        K.ver[a] = f->tpCam.vertical[a];
    }
    K.maxHistory = o.max_history;
    K.sigmaPlane = o.sigma_plane;
    K.normalCos = o.normal_cos;
    K.width = f->width;
    K.height = f->height;
    K.haveHistory = f->tpHave ? 1 : 0;
    K.linear = (o.flags & PT_TEMPORAL_LINEAR) ? 1 : 0;
    HIP_TRY(pt::temporalPass(src, aov, f->tpHist[f->tpCur].p, f->tpHist[f->tpCur ^ 1].p, dst, dlen, K, st));
    if (!on_dev) {   // synchronous: the history advances only when the caller has its result
        HIP_TRY(hipMemcpyAsync(out, f->tpRgb.p, np * 12, hipMemcpyDeviceToHost, st));
        if (out_len) HIP_TRY(hipMemcpyAsync(out_len, f->tpLen.p, np * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // The images take turns at enqueue time: the next call on this stream gathers from what this one writes.
    f->tpCur ^= 1;
    f->tpHave = true;
    f->tpCam = *cam;
    guard.ok = true;
    return PT_OK;
}

int pt_film_temporal_reset(pt_film* f) {
    if (!f) return fail(PT_ERR_INVALID, "pt_film_temporal_reset: null film");
    f->tpHave = false;
    return PT_OK;
}

int pt_render(pt_scene* s, pt_film* f, const pt_camera* cam, int spp, int max_depth, float* out, int on_dev,
              void* stream, pt_stats* stats) {
    return pt_render_ex(s, f, cam, spp, max_depth, out, on_dev, stream, nullptr, stats);
}

int pt_render_ex(pt_scene* s, pt_film* f, const pt_camera* cam, int spp, int max_depth, float* out, int on_dev,
                 void* stream, const pt_render_opts* opts, pt_stats* stats) {
    if (!s || !f || !cam || !out || spp <= 0) return fail(PT_ERR_INVALID, "pt_render: bad argument");
    if (!s->built) return fail(PT_ERR_STATE, "pt_render: BVH not built");
    if (s->device != f->device) return fail(PT_ERR_INVALID, "pt_render: scene and film on different devices");
    if (!(cam->lens_radius >= 0.0f) || !std::isfinite(cam->lens_radius))
        return fail(PT_ERR_INVALID, "pt_render: lens radius must be finite and >= 0");
    int rc = setDevice(s->device);
    if (rc) return rc;
    pt::RenderFacts facts = renderFacts(s, f, cam, spp, max_depth, opts);
    pt::RenderOptions o;
    if ((rc = pt::resolveRenderOptions(facts, o))) return rc;
    if (o.kernel == PT_KERNEL_WIDE && (rc = ensureWide(s))) return rc;   // (first use: builds the tree)
    facts = renderFacts(s, f, cam, spp, max_depth, opts);                // (the wide tree's depth and records)
    pt::RenderPlan plan;
    if ((rc = pt::planRender(facts, o, plan))) return rc;
    if (o.kernel == PT_KERNEL_WIDE && s->nobj > 0 && (!s->wide.p || !(plan.triRecords ? s->wtris.p : s->wprims.p)))
        return fail(PT_ERR_STATE, "wide BVH missing");
    RenderCall c;
    c.st = on_dev ? (hipStream_t)stream : 0;
    c.outBpp = o.fmt == PT_OUT_RGB32F ? 12 : 4;
    c.dst = out;
    if ((rc = reserveFilm(s, f, o, plan, on_dev != 0, c))) return rc;
    RenderParams P;
    fillRenderParams(P, s, f, cam, spp, max_depth, o, plan, c);
    if ((rc = enqueueFrame(f, P, spp, o, plan, c))) return rc;
    if ((rc = sortNextLaunch(f, o, plan, c.st))) return rc;
    if ((rc = dumpDiagnostics(f, plan, c))) return rc;
    const int64_t np = f->npix;
    if (!on_dev && np > 0) HIP_TRY(hipMemcpy(out, c.dst, np * c.outBpp, hipMemcpyDeviceToHost));
    // With stats (or a host output) the call waits for the frame; without, it returns at once.
    if (stats || !on_dev) return filmStats(f, stats);
    return PT_OK;
}

int pt_film_stats(pt_film* f, pt_stats* stats) {
    if (!f || !stats) return fail(PT_ERR_INVALID, "pt_film_stats: null argument");
    int rc = setDevice(f->device);
    if (rc) return rc;
    return filmStats(f, stats);
}

void pt_film_destroy(pt_film* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

void pt_scene_destroy(pt_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

}  // extern "C"
#endif  // PT_TU_COMPAT
