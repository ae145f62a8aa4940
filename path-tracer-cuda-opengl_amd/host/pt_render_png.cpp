// pt_render_png — command-line renderer, the counterpart of the reference's main() ->
// renderToPng() (main.cu:462-487, 530-535): build a scene, build the LBVH, initialise the
// per-pixel RNG streams, render, quantise and write a PNG.  Runtime flags replace the
// reference's compile-time constants (global_variables.h:28-35, macros.h:8-12).
// With --gpus N the frame is split into interleaved row stripes, one host thread per GPU.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "pt.h"

static void usage() {
    std::fprintf(stderr,
                 "usage: pt_render_png [--scene NAME] [--models DIR] [--width W] [--height H] [--spp N]\n"
                 "                     [--depth D] [--seed S] [--gpus N] [--stripe ROWS] [--out FILE]\n"
                 "                     [--rng compat|sample] [--frames K] [--sky default|black] [--nee] [--mis]\n"
                 "                     [--denoise] [--denoise-sigma X]\n"
                 "--frames K: progressive rendering, K frames of --spp samples accumulated per pixel (the\n"
                 "            headless counterpart of the reference's interactive loop); PNG of the last one\n"
                 "--sky: the sky the scene is rendered under; without it the preset's own (pt_preset_sky):\n"
                 "       black for the _lit scenes, whose lamp emits, the reference's gradient otherwise\n"
                 "--nee: next-event estimation (PT_RENDER_NEE): sample the emissive triangles directly at every\n"
                 "       Lambertian hit; off by default; changes nothing in a scene without emissive triangles\n"
                 "--mis: next-event estimation with multiple importance sampling (PT_RENDER_MIS; implies --nee):\n"
                 "       the light sample and the scatter ray weighted by their pdfs (balance heuristic), so the\n"
                 "       light term next to a lamp is bounded instead of clamped\n"
                 "--denoise: filter the frame before the PNG (pt_render_aov + pt_film_denoise: the a-trous filter\n"
                 "       guided by first-hit albedo, normal and position, 5 passes); its colour tolerance is\n"
                 "       1.2 / sqrt(accumulated samples per pixel) unless --denoise-sigma X gives it; one GPU only\n"
                 "scenes: triangle_world (default, as the reference), random_world, test_world, rtiow,\n"
                 "        cornell, bunny_cornell, bunny_field, cornell_lit, bunny_cornell_lit\n");
}

#define CHECK(x)                                                                      \
    do {                                                                              \
        int _rc = (x);                                                                \
        if (_rc != PT_OK) {                                                           \
            std::fprintf(stderr, "%s failed (%d): %s\n", #x, _rc, pt_last_error());   \
            std::exit(99);                                                            \
        }                                                                             \
    } while (0)

int main(int argc, char** argv) {
    std::string scene = "triangle_world", models = "models", out = "debug.png", sky;
    int width = 0, height = 0, spp = -1, depth = -1, gpus = 1, stripe = 8, frames = 1, rng = PT_RNG_COMPAT;
    bool nee = false, mis = false, denoise = false;
    float denoiseSigma = 0.0f;
    unsigned long long seed = 1;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { usage(); std::exit(2); }
            return argv[++i];
        };
        if (a == "--scene") scene = next();
        else if (a == "--models") models = next();
        else if (a == "--width") width = std::atoi(next());
        else if (a == "--height") height = std::atoi(next());
        else if (a == "--spp") spp = std::atoi(next());
        else if (a == "--depth") depth = std::atoi(next());
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--stripe") stripe = std::atoi(next());
        else if (a == "--out") out = next();
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--nee") nee = true;
        else if (a == "--mis") mis = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-sigma") {
            denoiseSigma = (float)std::atof(next());
            if (!(denoiseSigma > 0.0f) || !std::isfinite(denoiseSigma)) { usage(); return 2; }
        }
        else if (a == "--sky") {
            sky = next();
            if (sky != "default" && sky != "black") { usage(); return 2; }
        }
        else if (a == "--rng") {
            std::string r = next();
            if (r == "compat") rng = PT_RNG_COMPAT;
            else if (r == "sample") rng = PT_RNG_SAMPLE;
            else { usage(); return 2; }
        }
        else { usage(); return 2; }
    }
    if (denoise && gpus > 1) {   // (the guides of a pixel's taps live on other GPUs: gathering them is out of scope)
        usage();
        return 2;
    }
    pt_scene_desc d;
    CHECK(pt_preset_scene(scene.c_str(), models.c_str(), width, height, &d));
    if (spp > 0) d.spp = spp;
    if (depth >= 0) d.max_depth = depth;
    // the sky: the preset's own, or --sky's ("default" = the reference's gradient, main.cu:34-36)
    float horizon[3] = {1.0f, 1.0f, 1.0f}, zenith[3] = {0.5f, 0.7f, 1.0f};
    if (sky.empty()) CHECK(pt_preset_sky(scene.c_str(), horizon, zenith));
    if (sky == "black")
        for (int a = 0; a < 3; a++) horizon[a] = zenith[a] = 0.0f;
    int ndev = 0;
    CHECK(pt_device_count(&ndev));
    if (ndev <= 0) { std::fprintf(stderr, "no GPU visible\n"); return 99; }
    if (gpus > ndev) gpus = ndev;
    std::printf("scene %s: %lld objects, %dx%d @%dspp depth %d on %d GPU(s)\n", d.name, (long long)d.n_objects,
                d.width, d.height, d.spp, d.max_depth, gpus);

    if (frames < 1) frames = 1;
    // The frame is quantised on the device (PT_OUT_RGBA8: PngImage::saveColor per pixel), so each
    // GPU hands back 4 bytes per pixel of its row stripes.
    std::vector<uint8_t> frame((size_t)d.width * d.height * 4);
    std::vector<pt_stats> stats(gpus);
    std::vector<double> kms(gpus, 0.0);
    std::vector<std::thread> th;
    auto t0 = std::chrono::steady_clock::now();
    for (int g = 0; g < gpus; g++) {
        th.emplace_back([&, g]() {
            pt_scene* s = nullptr;
            pt_film* f = nullptr;
            CHECK(pt_scene_create(g, d.objects, d.n_objects, d.materials, d.n_materials, &s));
            CHECK(pt_scene_set_sky(s, horizon, zenith));
            CHECK(pt_scene_build_bvh(s, PT_BVH_ORIGIN_BOUNDS));
            CHECK(pt_film_create(g, d.width, d.height, stripe, gpus, g, seed, &f));
            int nrows = 0;
            int64_t npix = 0;
            CHECK(pt_film_info(f, &nrows, &npix));
            std::vector<int32_t> rows(nrows);
            CHECK(pt_film_rows(f, rows.data()));
            std::vector<uint8_t> part((size_t)npix * 4);
            std::vector<float> rgb(denoise ? (size_t)npix * 3 : 0);   // --denoise: the frame as floats, filtered before it is quantised
            pt_render_opts o{};
            o.rng = rng;
            o.out_format = denoise ? PT_OUT_RGB32F : PT_OUT_RGBA8;
            o.flags = (frames > 1 ? PT_RENDER_ACCUMULATE : 0) | (nee ? PT_RENDER_NEE : 0) | (mis ? PT_RENDER_MIS : 0);
            pt_stats st{};
            for (int k = 0; k < frames; k++) {
                CHECK(pt_render_ex(s, f, &d.camera, d.spp, d.max_depth,
                                   denoise ? rgb.data() : reinterpret_cast<float*>(part.data()), 0, nullptr, &o, &st));
                kms[g] += st.kernel_ms;
                stats[g].rays += st.rays;
                if (frames > 1 && g == 0)
                    std::printf("frame %d: %d spp accumulated, %.2f ms kernel on GPU 0\n", k + 1, (k + 1) * d.spp,
                                st.kernel_ms);
            }
            if (denoise) {   // (one GPU, the whole frame) the guides, the filter, then PngImage::saveColor's quantisation
                std::vector<pt_aov> aov((size_t)npix);
                pt_stats ast{};
                CHECK(pt_render_aov(s, f, &d.camera, aov.data(), 0, nullptr, &ast));
                int64_t samples = (int64_t)frames * d.spp;
                if (frames > 1) CHECK(pt_film_accumulated(f, &samples));
                pt_denoise_opts dn{};
                dn.iterations = 5;
                dn.sigma_color = denoiseSigma > 0.0f ? denoiseSigma : (float)(1.2 / std::sqrt((double)std::max<int64_t>(1, samples)));
                dn.sigma_albedo = 0.1f;
                dn.sigma_plane = 0.02f;
                CHECK(pt_film_denoise(f, rgb.data(), aov.data(), rgb.data(), 0, nullptr, &dn));
                std::printf("denoised: %lld spp, sigma_color %.4f, AOV pass %.3f ms kernel\n", (long long)samples,
                            dn.sigma_color, ast.kernel_ms);
                for (size_t i = 0; i < (size_t)npix; i++) {   // png_image.h:24-30, rows kept in film order
                    for (int c = 0; c < 3; c++) {
                        const float v = rgb[3 * i + c];
                        part[4 * i + c] = (uint8_t)((v < 0.0f ? 0.0f : v > 0.999f ? 0.999f : v) * 256.0f);
                    }
                    part[4 * i + 3] = 255;
                }
            }
            for (int r = 0; r < nrows; r++)
                std::memcpy(&frame[(size_t)rows[r] * d.width * 4], &part[(size_t)r * d.width * 4], 4 * (size_t)d.width);
            pt_film_destroy(f);
            pt_scene_destroy(s);
        });
    }
    for (auto& t : th) t.join();
    double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    unsigned long long rays = 0;
    double kmax = 0;
    for (int g = 0; g < gpus; g++) {
        rays += stats[g].rays;
        kmax = kms[g] > kmax ? kms[g] : kmax;
    }
    std::printf("Time Cost: %.3f s kernel (max over GPUs), %.3f s wall incl. setup; %.1f Mray/s\n", kmax / 1e3, wall,
                rays / (kmax * 1e3));
    CHECK(pt_write_png_rgba8(out.c_str(), frame.data(), d.width, d.height));
    pt_scene_desc_free(&d);
    return 0;
}
