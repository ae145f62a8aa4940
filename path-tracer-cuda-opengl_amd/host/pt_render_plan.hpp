// pt_render_plan.hpp — what pt_render_ex decides before it touches the device: the options of a
// call (explicit `opts` win, then the environment, then the defaults) and the launch they lead to
// (kernel, stack, thresholds, sample-mode tasks, critical pixels, split tiles, grid).  Plain host
// arithmetic on plain values, no HIP: csrc/pt_device.hip includes it (so `make variant DEFS=...`
// reaches the knobs below), and tests/cpp/render_plan_check.cpp runs it on a CPU
// (tests/test_render_plan_host.py).  Environment knobs are read on every call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pt.h"
#include "pt_error.hpp"
#include "pt_instancing.hpp"   // wideStackFor
#include "pt_wide8.hpp"        // kW8FarExt

// ------------------------------------------------------------------ compile-time knobs
// compat critical pixels: how many (PT_CRIT_PIXELS) and how many per wave (PT_CRIT_LANES)
#ifndef PT_CRIT_PIXELS
#define PT_CRIT_PIXELS 256
#endif
#ifndef PT_CRIT_LANES
#define PT_CRIT_LANES 4
#endif
#ifndef PT_TASK_POOL
#define PT_TASK_POOL 64
#endif
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 32   // sample mode: traversal stack entries per lane kept in LDS
#endif
// Instanced scenes draw the far line at 2 world extents: their mesh trees are quantised for origins
// within that reach (buildInstanced), 4x finer planes than 8 extents would allow (c5i 503 -> 498
// ms); farther origins start at their entry into the world (instEntry).
#ifndef PT_INST_FAR_EXT
#define PT_INST_FAR_EXT 2.0f
#endif

namespace pt {

constexpr int kCritPixels = PT_CRIT_PIXELS;
constexpr int kCritLanes = PT_CRIT_LANES;
constexpr int kTaskPool = PT_TASK_POOL;   // sample mode: tasks a wave reserves per atomic
constexpr float kInstFarExt = PT_INST_FAR_EXT;
// which compat kernels have critical-pixel waves: the flattened wide tree on shallow trees (stack 8:
// the 4-waves/SIMD compat kernels, whose 128-VGPR budget holds the per-lane loop without spills)
// (constexpr: the kernels' template text reads it as well)
constexpr bool critFor(bool sample, bool wide, bool inst, int stack) {
    return !sample && wide && !inst && stack <= 8;
}
// The stacks the AHEAD instantiations exist for (kAheadFor, csrc/pt_device.hip)
constexpr bool aheadStack(int stack) { return stack == 8 || stack == 16; }

// The binary tree's stack entries for a depth (the wide tree's: wideStackFor, pt_instancing.cpp)
inline int stackFor(int depth) {
    const int need = depth + 1;
    for (int s : {16, 24, 32, 48, 64, 80})
        if (need <= s) return s;
    return -1;
}

// A threshold knob in lanes: 1..64; unset, unparsable or "0": the default.
inline int envInt(const char* name, int dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    int x = std::atoi(v);
    if (x < 1) return dflt;   // "0": the default
    return x > 64 ? 64 : x;
}
// A count knob: any value >= 0 (0 is zero, not the default); unset or unparsable: the default.
inline int envCount(const char* name, int dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    const long x = std::strtol(v, &end, 10);
    if (end == v || x < 0) return dflt;
    return (int)std::min<long>(x, 1L << 30);
}

// ------------------------------------------------------------------ inputs
// What the decisions read of the scene, the film and the call, by value.
struct RenderFacts {
    // scene
    bool instanced = false, instLights = false, hasSpheres = false, hasEmissive = false, lambertOnly = true;
    bool wideReady = false, haveWtris = false;
    int64_t nobj = 0, nLights = 0;
    int depth = 0, wideDepth = 0;   // (wideDepth: valid once the wide tree exists, i.e. for planRender)
    float sceneCE[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float skyH[3] = {1.0f, 1.0f, 1.0f}, skyZ[3] = {0.5f, 0.7f, 1.0f};
    // film
    int width = 0, height = 0, nrows = 0, stripe_h = 1;
    int64_t npix = 0;
    bool haveOrder = false;
    int framesSinceCost = 0, critK = 0;
    int64_t accumSamples = 0;
    // call
    const pt_camera* cam = nullptr;
    int spp = 0, max_depth = 0;
    const pt_render_opts* opts = nullptr;
};

// ------------------------------------------------------------------ stage 1: the options
struct RenderOptions {
    int fmt = PT_OUT_RGB32F;
    bool accumulate = false;
    bool nee = false, mis = false;   // the flags, on a scene with sampled lights
    int kernel = PT_KERNEL_WIDE;     // resolved: never PT_KERNEL_DEFAULT
    int rng = PT_RNG_COMPAT;
    bool lpt = true;                 // longest tiles first (not PT_RENDER_IDENTITY_ORDER)
};

// Resolves and validates the options of a call.  Needs no wide tree (pt_render_ex builds it, at
// first use, only for a call that passes these checks).
inline int resolveRenderOptions(const RenderFacts& F, RenderOptions& o) {
    const pt_render_opts* opts = F.opts;
    o.fmt = opts ? opts->out_format : PT_OUT_RGB32F;
    if (o.fmt != PT_OUT_RGB32F && o.fmt != PT_OUT_RGBA8 && o.fmt != PT_OUT_RGBA8_SURFACE)
        return fail(PT_ERR_INVALID, "pt_render_ex: unknown output format");
    o.accumulate = opts && (opts->flags & PT_RENDER_ACCUMULATE);
    const bool misFlag = opts && (opts->flags & PT_RENDER_MIS);   // (implies PT_RENDER_NEE)
    const bool neeFlag = misFlag || (opts && (opts->flags & PT_RENDER_NEE));
    if (o.accumulate && F.accumSamples + F.spp >= (1ll << 24))
        return fail(PT_ERR_INVALID, "pt_render_ex: accumulated samples must stay below 2^24");
    // Kernel choice and wavefront-scheduler thresholds (lanes of 64): explicit options win, then
    // the PT_RENDER_KERNEL / PT_LEAF_BATCH / PT_SHADE_BATCH environment (tuning), then defaults.
    o.kernel = opts ? opts->kernel : PT_KERNEL_DEFAULT;
    if (o.kernel == PT_KERNEL_DEFAULT) {
        const char* k = std::getenv("PT_RENDER_KERNEL");
        const std::string ks = k ? k : "";
        o.kernel = ks == "simple" ? PT_KERNEL_SIMPLE : (ks == "wavefront" ? PT_KERNEL_WAVEFRONT : PT_KERNEL_WIDE);
    }
    if (o.kernel != PT_KERNEL_SIMPLE && o.kernel != PT_KERNEL_WAVEFRONT && o.kernel != PT_KERNEL_WIDE)
        return fail(PT_ERR_INVALID, "pt_render_ex: unknown kernel");
    if (F.instanced && o.kernel != PT_KERNEL_WIDE)
        return fail(PT_ERR_INVALID, "pt_render_ex: instanced scenes render with the wide kernel (PT_KERNEL_WIDE)");
    if (misFlag && F.instanced && !F.instLights)   // (an instanced scene lists its lights on request: PT_BVH_LIGHTS)
        return fail(PT_ERR_INVALID, "pt_render_ex: PT_RENDER_MIS is not available on instanced scenes (flat scenes only)");
    if (misFlag && o.kernel == PT_KERNEL_WAVEFRONT)
        return fail(PT_ERR_INVALID, "pt_render_ex: PT_RENDER_MIS is not available with PT_KERNEL_WAVEFRONT "
                                    "(PT_KERNEL_WIDE, PT_KERNEL_DEFAULT or PT_KERNEL_SIMPLE)");
    if (neeFlag && F.instanced && !F.instLights)
        return fail(PT_ERR_INVALID, "pt_render_ex: PT_RENDER_NEE is not available on instanced scenes (flat scenes only)");
    if (neeFlag && o.kernel == PT_KERNEL_WAVEFRONT)
        return fail(PT_ERR_INVALID, "pt_render_ex: PT_RENDER_NEE is not available with PT_KERNEL_WAVEFRONT "
                                    "(PT_KERNEL_WIDE, PT_KERNEL_DEFAULT or PT_KERNEL_SIMPLE)");
    o.nee = neeFlag && F.nLights > 0;   // (no sampled light: the flag changes nothing)
    o.mis = misFlag && o.nee;
    o.rng = opts ? opts->rng : PT_RNG_COMPAT;
    if (o.rng != PT_RNG_COMPAT && o.rng != PT_RNG_SAMPLE) return fail(PT_ERR_INVALID, "pt_render_ex: unknown rng mode");
    o.lpt = !(opts && (opts->flags & PT_RENDER_IDENTITY_ORDER));
    return PT_OK;
}

// ------------------------------------------------------------------ stage 2: the launch
// The 32-bit task counter (PT_TAKE_TASKS) runs past ntasks: every persistent wave takes
// exactly one pool of kTaskPool = 64 after the tasks are gone (its lanes each ask once more
// and share it), so the counter ends at ntasks + 64 * nwaves and must not wrap on the way --
// a wrapped grab would hand out task 0 again.  The limit leaves room for kMaxPersistentWaves
// such pools whatever the device (pt.h states it); the launch's nwaves is checked by persistentWaves.
constexpr uint64_t kMaxPersistentWaves = 1ull << 20;
constexpr uint64_t kTaskLimit = (1ull << 32) - (uint64_t)kTaskPool * kMaxPersistentWaves;   // 2^32 - 2^26

struct RenderPlan {
    int stack = 0;                        // traversal stack entries: the kernel instantiation
    bool triRecords = false;              // the scene has edge-form triangle records (DevScene::wprims reads them)
    int tri = 0, ahead = 0, lit = 0, camFar = 0;
    int leafBatch = 0, shadeBatch = 0, nodeMin = 0;
    int tiles_x = 0, ntiles = 0;
    bool sample = false;                  // sample rng on a film with pixels
    int block = 0, nblocks = 0, blockShift = -1, span = 0, ngroups = 0, nblocksShift = -1;
    uint32_t ntasks = 0;
    bool critOn = false;                  // this launch counts rays per pixel and selects the next one's critical pixels
    int nCrit = 0, critLanes = 0, critWaves = 0;
    int splitWays = 1, splitTiles = 0, compatGrid = 0;
    int prioTiles = 0, prioLevel = 0, measureCost = 0;
    bool sortTiles = false;               // the launch measures tile costs: the next ones' order is sorted after it
    bool resolve = false;
    int rawOut = 0;
    uint32_t sampleBase = 0;
    int stripeShift = -1;
    int spillEntries = 0;                 // stack entries per lane beyond LDS (0: none)
    // Deep trees: stack entries beyond kLdsStack live in memory, per wave slot (persistent wave or
    // compat tile) and lane of 64
    size_t stackSpillBytes(size_t slots) const { return slots * 64u * (size_t)spillEntries * 4; }
};

inline int planRender(const RenderFacts& F, const RenderOptions& o, RenderPlan& p) {
    const pt_render_opts* opts = F.opts;
    const pt_camera* cam = F.cam;
    const int kernel = o.kernel;
    const bool nee = o.nee, lpt = o.lpt;
    const int64_t np = F.npix;
    p = RenderPlan();
    // (the render kernels' triangle-only LEAF path reads edge-form records: DevScene::wprims)
    // The kernels' TRI instantiations read nothing else, so they launch under this one condition
    // (PT_WIDE_TRI=0: the generic kernels on the same records, for tests and same-library A/B runs).
    p.triRecords = F.wideReady && F.haveWtris && !F.hasSpheres && !F.instanced;
    p.tri = p.triRecords && kernel == PT_KERNEL_WIDE && envCount("PT_WIDE_TRI", 1) != 0 ? 1 : 0;
    {   // the LIT kernels only where they are needed: an emitter, or a sky that is not the reference's
        static const float H0[3] = {1.0f, 1.0f, 1.0f}, Z0[3] = {0.5f, 0.7f, 1.0f};
        p.lit = (F.hasEmissive || std::memcmp(F.skyH, H0, sizeof(H0)) != 0 || std::memcmp(F.skyZ, Z0, sizeof(Z0)) != 0) ? 1 : 0;
    }
    p.stripeShift = (F.stripe_h & (F.stripe_h - 1)) == 0 ? __builtin_ctz((unsigned)F.stripe_h) : -1;
    p.tiles_x = (F.width + 7) / 8;
    p.ntiles = p.tiles_x * ((F.nrows + 7) / 8);
    {   // the kernels' wideFar / instFar test for the camera: its rays then take the reference-order path
        // (instanced scenes: start at their entry into the world, instEntry).  A lens sample moves
        // the origin by lens * (x right + y up) with x^2 + y^2 < 1, i.e. by at most
        // lens * (|right_a| + |up_a|) on axis a, whatever right / up the caller filled in.
        double m = 0.0;
        for (int a = 0; a < 3; a++)
            m = std::max(m, std::fabs((double)cam->origin[a] - (double)F.sceneCE[a]) +
                                (double)cam->lens_radius * (std::fabs((double)cam->right[a]) + std::fabs((double)cam->up[a])));
        p.camFar = !(m <= (F.instanced ? (double)kInstFarExt : (double)kW8FarExt) * (double)F.sceneCE[3]) ? 1 : 0;
    }
    // Defaults swept on C3 (tools/ab_env.py): sample mode is throughput-bound and prefers full
    // LEAF / SHADE steps.  Compat mode on the binary tree is bound by its slowest pixels' sequential
    // chains: 20 / 12 together with nodeMin 8 (C3 1,521 -> 1,442 ms, C2 90.7 -> 80.0, C5 1,311 ->
    // 1,180 against 8 / 12).  Compat on the flattened wide tree, since round 6 (its critical chains
    // in critical-pixel waves, or short paths): the sample mode's wide thresholds with nodeMin 8 --
    // C3 @1024 (critical pixels on) 705 -> 649 ms (SHADE 28 alone 665, 20 674; LEAF 28 alone 695),
    // C5 @512 558 -> 539 (24 / 24), C2 @256 37.7 -> 37.1; nodeMin 0 740 / 617 ms, 4: 656 on C3.
    const bool sampleRng = o.rng == PT_RNG_SAMPLE;
    // sample mode, wide kernel (speculative traversal): LEAF at 28 waiting lanes, SHADE at 28
    // (C3 @256 spp 148.4 -> 145.0 ms vs 24 / 32; C5 @64 75.9 -> 74.5; C2 @1024 135.4 -> 134.5);
    // deep wide trees (a 16+ entry stack: C5's 1.04 M triangles) at 24 / 24 (round 3 close: C5 @64
    // 67.1 -> 65.1 ms, median of 5; C3 at 24 / 24 is 1 % slower, so shallow trees keep 28 / 28)
    const bool wideSample = sampleRng && kernel == PT_KERNEL_WIDE;
    const bool wideFlatCompat = !sampleRng && kernel == PT_KERNEL_WIDE && !F.instanced;
    const int stack = kernel == PT_KERNEL_WIDE ? wideStackFor(F.wideDepth) : (F.nobj > 1 ? stackFor(F.depth) : 16);
    p.stack = stack;
    const int wideBatch = stack >= 16 ? 24 : 28;
    // instanced scenes (no speculative traversal: a lane with primitives waiting cannot visit nodes)
    // take their LEAF steps earlier: LEAF 16 / SHADE 20 (round 5, C5 instanced @128 spp, interleaved
    // median of 3: 131.8 -> 128.8 ms; LEAF 12: 131.8, 8: 135.9, 32: 140.7; SHADE 28 with LEAF 16: 131.4)
    // (instanced compat takes them too: C5 instanced compat @512 618.6 -> 594.6 ms; 24 / 24: 609.8,
    // 28 / 28: 646.5)
    const bool instWide = kernel == PT_KERNEL_WIDE && F.instanced;
    p.leafBatch = (opts && opts->leaf_batch > 0) ? std::min(opts->leaf_batch, 64)
                                                 : envInt("PT_LEAF_BATCH", instWide ? 16 : (wideSample || wideFlatCompat) ? wideBatch
                                                                                                       : (sampleRng ? 24 : 20));
    // compat mode: a NODE step with fewer than nodeMin lanes yields to the larger of the waiting
    // LEAF / SHADE groups (C3 compat 1,620 -> 1,517 ms at 8; 4: 1,548, 16: 1,671, 32: 1,989)
    p.nodeMin = std::getenv("PT_NODE_MIN") ? std::atoi(std::getenv("PT_NODE_MIN")) : 8;
    p.shadeBatch = (opts && opts->shade_batch > 0) ? std::min(opts->shade_batch, 64)
                                                   : envInt("PT_SHADE_BATCH", instWide ? 20 : (wideSample || wideFlatCompat) ? wideBatch
                                                                                                           : (sampleRng ? 32 : 12));
    if (kernel == PT_KERNEL_SIMPLE) p.leafBatch = 0;
    const bool sample = sampleRng && np > 0 && p.ntiles > 0;
    p.sample = sample;
    // The AHEAD kernels: a triangle-only flat scene in sample mode on the wide kernel, no material that
    // draws outside the unit-sphere loop, a pinhole camera, no light sampling, a stack they are built for
    // (PT_SHADE_AHEAD=0: today's kernels in the same library, for tests and A/B runs).
    p.ahead = sample && p.tri && F.lambertOnly && cam->lens_radius == 0.0f && !nee && aheadStack(stack) &&
                      envCount("PT_SHADE_AHEAD", 1) != 0 ? 1 : 0;
    // compat critical pixels (wide kernel, flattened scene, long paths): the previous launch's
    // PT_CRIT_PIXELS longest per-pixel chains run first, PT_CRIT_LANES pixels per wave, each lane
    // tracing its rays in one per-lane loop (a lane alone on its chain is not held back by the wave's
    // step kinds).  C3 compat @1024 (interleaved, median of 2): 773 ms without; 256 x 4 699 ms;
    // 64 x 1 710, 128 x 4 707, 512 x 4 712, 256 x 8 751 (with the split tiles as well).  The rays
    // per pixel are measured on every launch.
    p.critLanes = std::max(1, std::min(64, envCount("PT_CRIT_LANES", kCritLanes)));
    // (not in NEE launches: the per-lane loop knows no shadow query; the waves only schedule)
    p.critOn = lpt && !nee && critFor(sample, kernel == PT_KERNEL_WIDE, F.instanced, stack) && np > 0 &&
               F.max_depth > 16 && envCount("PT_CRIT_PIXELS", kCritPixels) > 0;
    if (p.critOn && F.critK > 0) {
        p.nCrit = F.critK;
        p.critWaves = (p.nCrit + p.critLanes - 1) / p.critLanes;
    }
    // compat tile waves: the longest tiles of the launch order split into splitWays waves (renderKernelWF).
    // Only where a pixel's sequential chain can outlast the frame's throughput-bound part: long paths
    // (max_depth > 16; C3, depth 50: 800 -> 766 ms) on kernels without critical-pixel waves, which
    // take those chains out of the tile waves (C3 with both: 710 ms, critical pixels alone 699 ms).
    // Short-path frames are throughput-bound and the split's idle lanes cost (C5, depth 16: 548 ->
    // 553 ms; C2, depth 8: +0.9 %).
    p.splitWays = std::max(1, std::min(8, envCount("PT_SPLIT_WAYS", 2)));
    p.splitTiles = (lpt && F.haveOrder && !sample && kernel != PT_KERNEL_SIMPLE)
                       ? std::max(0, std::min(p.ntiles, envCount("PT_SPLIT_TILES", F.max_depth > 16 && !p.critOn ? 128 : 0))) : 0;
    if (p.splitWays == 1) p.splitTiles = 0;
    p.compatGrid = p.critWaves + p.ntiles + p.splitTiles * (p.splitWays - 1);
    // diagnostic: only the first k waves of the launch order (the longest tiles) -- their chains'
    // latency with the machine otherwise idle; the other pixels are not rendered
    if (const int lim = envCount("PT_COMPAT_GRID_LIMIT", 0)) p.compatGrid = std::min(p.compatGrid, lim);
    if (sample) {
        if (F.width >= 65536 || F.nrows >= 65536)
            return fail(PT_ERR_INVALID, "sample mode: frame width and rows must be < 65536");
        p.block = (opts && opts->chunk > 0) ? opts->chunk : std::max(16, (F.spp + 63) / 64);
        p.nblocks = (F.spp + p.block - 1) / p.block;
        p.blockShift = (p.block & (p.block - 1)) == 0 ? __builtin_ctz((unsigned)p.block) : -1;
        p.span = p.block;   // one summation block per task
        p.ngroups = p.nblocks;
        const uint64_t ntasks = (uint64_t)p.ntiles * (uint64_t)p.ngroups * 64u;
        if (ntasks >= kTaskLimit)
            return fail(PT_ERR_INVALID, "sample mode: too many (pixel, block) tasks (tiles x blocks x 64 must stay "
                                        "below 2^32 - 2^26); raise the block size (chunk)");
        p.ntasks = (uint32_t)ntasks;
        // the launch order decoded per slot (tileXYKernel) divides by ngroups
        p.nblocksShift = (p.ngroups & (p.ngroups - 1)) == 0 ? __builtin_ctz((unsigned)p.ngroups) : -1;
        // Tile costs (rays of the tile's most expensive pixel) are measured on the first frame and
        // then on one frame in eight: the order only steers the launch's tail, and counting costs
        // one more atomic per task.
        p.measureCost = (lpt && (!F.haveOrder || F.framesSinceCost >= 7)) ? 1 : 0;
    }
    if (kernel == PT_KERNEL_WAVEFRONT && stack > PT_LDS_STACK && p.ntiles > 0) p.spillEntries = stack - PT_LDS_STACK;
    // A resolve pass follows the render kernel in sample mode (block sums) and whenever the film
    // accumulates or the output is 8-bit; compat kernels then store raw sums into the film's `sums`.
    p.resolve = np > 0 && (sample || o.accumulate || o.fmt != PT_OUT_RGB32F);
    p.rawOut = p.resolve && !sample ? 1 : 0;
    if (o.accumulate && sample) p.sampleBase = (uint32_t)F.accumSamples;   // frames continue the sample sequence
    p.prioTiles = (lpt && F.haveOrder && !sample) ? envCount("PT_PRIO_TILES", 1024) : 0;
    p.prioLevel = std::max(1, std::min(3, envCount("PT_PRIO_LEVEL", 2)));
    p.sortTiles = lpt && p.ntiles > 0 && (!sample || p.measureCost);
    return PT_OK;
}

// Persistent waves (sample mode): exactly the waves that fit at once -- `perCU`, the kernel's
// occupancy per CU, which the LDS stack caps on deep trees -- and no more than the tasks fill.
inline int persistentWaves(int cus, int perCU, uint64_t ntasks, int& nwaves) {
    nwaves = (int)std::min<uint64_t>((uint64_t)cus * (uint64_t)std::max(1, perCU), (ntasks + 63) / 64);
    return (uint64_t)nwaves > kMaxPersistentWaves
               ? fail(PT_ERR_STATE, "sample mode: more persistent waves than the task limit leaves room for") : PT_OK;
}

}  // namespace pt
