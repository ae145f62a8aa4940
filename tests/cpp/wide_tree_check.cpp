// Structural check of a wide tree given as files (TEST INFRASTRUCTURE: built by the package Makefile
// with the host compiler, run by tests/test_wide_tree_check.py and tests/test_gpu_wide_structure.py;
// the product never uses it).  The arrays are the ones pt_scene_download_wide returns for a flat
// scene, whichever builder wrote them (host/pt_wide8.cpp, csrc/pt_wide_build.hip SAH or PLOC).
//
//   wide_tree_check check objects.bin nodes.bin prims.bin depth slots capacity
//     recomputes the LBVH's leaf order, the leaf-order records and exact boxes and the reference
//     ranks from the objects as the library does (oracle keys and hierarchy, pt::primRecord,
//     pt::referenceRanks) and runs the checks of wide_tree_checks.hpp on the arrays.  nodes.bin may
//     hold more slots than `slots` reports (a mutated copy); the walk never reads beyond either.
//     Prints one summary line; exits 1 when a check failed (each printed under its name), 2 on
//     unusable input.
//   wide_tree_check build objects.bin nodes.bin prims.bin
//     builds the host tree with pt::buildWide8 from the same inputs, writes its arrays and prints
//     "depth <d> slots <s>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt.h"
#include "pt_wide8.hpp"
#include "wide_tree_checks.hpp"

extern "C" {
typedef struct { int32_t left, right, parent, objid; float bmin[3], bmax[3]; } orc_node;
int orc_morton_keys(const pt_object* objs, int64_t n, int include_origin, uint64_t* keys_out);
int orc_build_lbvh(const pt_object* objs, int64_t n, const uint64_t* keys, int tight, orc_node* nodes);
}

namespace {
template <class T>
bool readAll(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    const bool ok = n % (long)sizeof(T) == 0 && (n == 0 || std::fread(v.data(), 1, (size_t)n, f) == (size_t)n);
    std::fclose(f);
    return ok;
}
template <class T>
bool writeAll(const char* path, const std::vector<T>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (!((mode == "check" && argc == 8) || (mode == "build" && argc == 5))) {
        std::fprintf(stderr, "usage: wide_tree_check check objects.bin nodes.bin prims.bin depth slots capacity\n"
                             "       wide_tree_check build objects.bin nodes.bin prims.bin\n");
        return 2;
    }
    std::vector<pt_object> objs;
    if (!readAll(argv[2], objs) || objs.empty()) return 2;
    const int64_t n = (int64_t)objs.size();
    // the LBVH's leaf order, records and boxes (leafGatherKernel), the reference ranks (as wide8_check.cpp)
    std::vector<uint64_t> keys((size_t)n);
    orc_morton_keys(objs.data(), n, 1, keys.data());
    std::vector<orc_node> nd((size_t)(2 * n - 1));
    orc_build_lbvh(objs.data(), n, keys.data(), 1, nd.data());
    std::vector<uint32_t> leafPrims((size_t)n * 12, 0u);
    std::vector<float> boxes((size_t)n * 6);
    for (int64_t k = 0; k < n; k++) {
        const uint32_t id = (uint32_t)(keys[k] & 0xffffffffu);
        pt::primRecord(objs[id], id, &leafPrims[(size_t)k * 12], &boxes[(size_t)k * 6]);
    }
    std::vector<uint32_t> lref((size_t)std::max<int64_t>(1, n - 1)), rref(lref.size());
    for (int64_t i = 0; i + 1 < n; i++) {
        auto ref = [&](int32_t c) { return c >= n - 1 ? (0x80000000u | (uint32_t)(c - (n - 1))) : (uint32_t)c; };
        lref[(size_t)i] = ref(nd[(size_t)i].left);
        rref[(size_t)i] = ref(nd[(size_t)i].right);
    }
    const std::vector<uint32_t> rank = pt::referenceRanks(lref.data(), rref.data(), 1, n);

    if (mode == "build") {
        pt::Wide8 w;
        std::string err;
        if (!pt::buildWide8(leafPrims.data(), boxes.data(), rank.data(), n, w, err)) {
            std::fprintf(stderr, "build failed: %s\n", err.c_str());
            return 1;
        }
        if (!writeAll(argv[3], w.nodes) || !writeAll(argv[4], w.prims)) return 2;
        std::printf("depth %d slots %lld\n", w.depth, (long long)(w.nodes.size() / pt::kW8NodeDwords));
        return 0;
    }

    std::vector<uint32_t> nodes, prims;
    if (!readAll(argv[3], nodes) || !readAll(argv[4], prims)) return 2;
    widecheck::Report rep;
    rep.check(nodes.size() % pt::kW8NodeDwords == 0 && !nodes.empty(), "node array is whole slots", (long long)nodes.size());
    rep.check((int64_t)prims.size() == n * 12, "primitive array holds n records", (long long)prims.size(), n * 12);
    widecheck::WalkResult walk;
    if (rep.failures == 0) {
        const widecheck::WideArrays arrays{nodes.data(), (int64_t)(nodes.size() / pt::kW8NodeDwords), prims.data(), n,
                                           leafPrims.data(), boxes.data(), rank.data(), std::atoi(argv[5]),
                                           std::atoll(argv[6]), std::atoll(argv[7])};
        walk = widecheck::checkWideTree(arrays, rep);
    }
    rep.summary();
    std::printf("n %lld reached %lld leaves %lld depth %d emin %d failures %ld\n", (long long)n, (long long)walk.reached,
                (long long)walk.leaves, walk.depth, walk.emin, rep.failures);
    return rep.failures ? 1 : 0;
}
