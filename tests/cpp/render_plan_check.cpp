// render_plan_check — pt_render_ex's launch plan (host/pt_render_plan.hpp) on a CPU.
//
//   render_plan_check key=value ...          the facts of a call -> the resolved options and the plan,
//                                            one key=value per line; a refused call prints
//                                            error=<PT_ERR_* code> and message=<text> instead
//   render_plan_check waves cus perCU ntasks the persistent waves of a sample-mode launch (nwaves=...)
//
// Facts not given keep RenderFacts' defaults; the camera is all zero unless cam_x / cam_y / cam_z,
// lens, right_x.. / up_x.. say otherwise.  `opts` is NULL unless one of kernel, leaf_batch,
// shade_batch, flags, rng, chunk, out_format is given.  nwaves: the wave slots of a sample-mode
// launch, for spill_bytes (compat launches have compatGrid slots).  Environment knobs are read from
// the environment, as the library reads them.  Exit status 2 for an argument it does not know.
// tests/test_render_plan_host.py holds the expected values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pt_render_plan.hpp"

std::string& pt::lastError() {   // (the library's is in pt_host.cpp)
    static thread_local std::string e;
    return e;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "waves") == 0) {
        int nwaves = 0;
        const int rc = pt::persistentWaves(std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10), nwaves);
        if (rc) std::printf("error=%d\nmessage=%s\n", rc, pt::lastError().c_str());
        else std::printf("nwaves=%d\n", nwaves);
        return 0;
    }
    pt::RenderFacts F;
    pt_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    pt_render_opts opts;
    std::memset(&opts, 0, sizeof(opts));
    bool haveOpts = false;
    long long nwaves = 0;
    for (int k = 1; k < argc; k++) {
        const char* eq = std::strchr(argv[k], '=');
        if (!eq) return 2;
        const std::string key(argv[k], (size_t)(eq - argv[k]));
        const char* v = eq + 1;
        const long long i = std::strtoll(v, nullptr, 10);
        const float x = std::strtof(v, nullptr);
        if (key == "instanced") F.instanced = i != 0;
        else if (key == "instLights") F.instLights = i != 0;
        else if (key == "hasSpheres") F.hasSpheres = i != 0;
        else if (key == "hasEmissive") F.hasEmissive = i != 0;
        else if (key == "lambertOnly") F.lambertOnly = i != 0;
        else if (key == "wideReady") F.wideReady = i != 0;
        else if (key == "haveWtris") F.haveWtris = i != 0;
        else if (key == "nobj") F.nobj = i;
        else if (key == "nLights") F.nLights = i;
        else if (key == "depth") F.depth = (int)i;
        else if (key == "wideDepth") F.wideDepth = (int)i;
        else if (key == "centre_x") F.sceneCE[0] = x;
        else if (key == "centre_y") F.sceneCE[1] = x;
        else if (key == "centre_z") F.sceneCE[2] = x;
        else if (key == "extent") F.sceneCE[3] = x;
        else if (key == "skyH_x") F.skyH[0] = x;
        else if (key == "skyH_y") F.skyH[1] = x;
        else if (key == "skyH_z") F.skyH[2] = x;
        else if (key == "skyZ_x") F.skyZ[0] = x;
        else if (key == "skyZ_y") F.skyZ[1] = x;
        else if (key == "skyZ_z") F.skyZ[2] = x;
        else if (key == "width") F.width = (int)i;
        else if (key == "height") F.height = (int)i;
        else if (key == "nrows") F.nrows = (int)i;
        else if (key == "stripe_h") F.stripe_h = (int)i;
        else if (key == "npix") F.npix = i;
        else if (key == "haveOrder") F.haveOrder = i != 0;
        else if (key == "framesSinceCost") F.framesSinceCost = (int)i;
        else if (key == "critK") F.critK = (int)i;
        else if (key == "accumSamples") F.accumSamples = i;
        else if (key == "spp") F.spp = (int)i;
        else if (key == "max_depth") F.max_depth = (int)i;
        else if (key == "cam_x") cam.origin[0] = x;
        else if (key == "cam_y") cam.origin[1] = x;
        else if (key == "cam_z") cam.origin[2] = x;
        else if (key == "lens") cam.lens_radius = x;
        else if (key == "right_x") cam.right[0] = x;
        else if (key == "right_y") cam.right[1] = x;
        else if (key == "right_z") cam.right[2] = x;
        else if (key == "up_x") cam.up[0] = x;
        else if (key == "up_y") cam.up[1] = x;
        else if (key == "up_z") cam.up[2] = x;
        else if (key == "nwaves") nwaves = i;
        else {
            haveOpts = true;
            if (key == "kernel") opts.kernel = (int32_t)i;
            else if (key == "leaf_batch") opts.leaf_batch = (int32_t)i;
            else if (key == "shade_batch") opts.shade_batch = (int32_t)i;
            else if (key == "flags") opts.flags = (int32_t)i;
            else if (key == "rng") opts.rng = (int32_t)i;
            else if (key == "chunk") opts.chunk = (int32_t)i;
            else if (key == "out_format") opts.out_format = (int32_t)i;
            else return 2;
        }
    }
    F.cam = &cam;
    F.opts = haveOpts ? &opts : nullptr;
    pt::RenderOptions o;
    pt::RenderPlan p;
    int rc = pt::resolveRenderOptions(F, o);
    if (!rc) rc = pt::planRender(F, o, p);
    if (rc) {
        std::printf("error=%d\nmessage=%s\n", rc, pt::lastError().c_str());
        return 0;
    }
    std::printf("fmt=%d\naccumulate=%d\nnee=%d\nmis=%d\nkernel=%d\nrng=%d\nlpt=%d\n", o.fmt, o.accumulate ? 1 : 0, o.nee ? 1 : 0,
                o.mis ? 1 : 0, o.kernel, o.rng, o.lpt ? 1 : 0);
    std::printf("stack=%d\ntriRecords=%d\ntri=%d\nahead=%d\nlit=%d\ncamFar=%d\n", p.stack, p.triRecords ? 1 : 0, p.tri, p.ahead, p.lit,
                p.camFar);
    std::printf("leafBatch=%d\nshadeBatch=%d\nnodeMin=%d\ntiles_x=%d\nntiles=%d\n", p.leafBatch, p.shadeBatch, p.nodeMin, p.tiles_x,
                p.ntiles);
    std::printf("sample=%d\nblock=%d\nnblocks=%d\nblockShift=%d\nspan=%d\nngroups=%d\nnblocksShift=%d\nntasks=%u\n", p.sample ? 1 : 0,
                p.block, p.nblocks, p.blockShift, p.span, p.ngroups, p.nblocksShift, p.ntasks);
    std::printf("critOn=%d\nnCrit=%d\ncritLanes=%d\ncritWaves=%d\nsplitWays=%d\nsplitTiles=%d\ncompatGrid=%d\n", p.critOn ? 1 : 0,
                p.nCrit, p.critLanes, p.critWaves, p.splitWays, p.splitTiles, p.compatGrid);
    std::printf("prioTiles=%d\nprioLevel=%d\nmeasureCost=%d\nsortTiles=%d\n", p.prioTiles, p.prioLevel, p.measureCost,
                p.sortTiles ? 1 : 0);
    std::printf("resolve=%d\nrawOut=%d\nsampleBase=%u\nstripeShift=%d\n", p.resolve ? 1 : 0, p.rawOut, p.sampleBase, p.stripeShift);
    std::printf("spill_bytes=%zu\n", p.stackSpillBytes(p.sample ? (size_t)nwaves : (size_t)p.compatGrid));
    return 0;
}
