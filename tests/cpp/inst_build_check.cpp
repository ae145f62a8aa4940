// CPU check of the instanced scene's host tree build (host/pt_instancing.cpp) (TEST
// INFRASTRUCTURE: compiled and run by tests/test_inst_build.py; the product never uses it).
// Reads objects, mesh ranges, instances and materials, runs pt::buildInstancedTree twice and checks
// the two-level tree: every (instance, mesh primitive) pair reachable from slot 0 exactly once, the
// instance records' fields, the top-level entries' boxes (decoded from the parent's quantised
// planes, as nodeChildren does) around the fp64 world image of what lies below them, the layout
// and the scalars.  A failed build prints "rc <code>: <message>" and exits 3.
// usage: inst_build_check objects.bin meshes.bin instances.bin materials.bin dynamic rebraid budget
//
// With five more arguments it checks arrays downloaded from a scene on the device
// (pt_scene_download_wide: PT_WIDE_NODES and PT_WIDE_INSTANCES, pt_scene_wide_info's depth and
// slots) in place of the ones it built (tests/test_gpu_wide_structure.py; the package Makefile
// builds tools/micro/inst_build_check for it).  It still runs the host build on the scene files,
// which gives the layout (topCap, meshRoot, the entries) and the rows expected for these matrices:
//   ... nodes.bin winst.bin depth slots full   the arrays of a full build (source 3): byte for byte the host's
//   ... nodes.bin winst.bin depth slots top    after pt_scene_update_instances and a rebuild of the top
//       level on the device (source 4; instances.bin holds the new matrices): the rows are the host's,
//       and the walk above runs on the downloaded nodes, whose mesh trees are the first build's.
// In both the reported depth must be the walk's (top levels + the marker + the deepest mesh tree + 1)
// and the reported slots the layout's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt.h"
#include "pt_error.hpp"
#include "pt_instancing.hpp"

std::string& pt::lastError() {   // (the library's is in pt_host.cpp)
    static thread_local std::string e;
    return e;
}

namespace {
template <class T>
std::vector<T> readAll(const char* path) {
    std::vector<T> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (n > 0 && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
    std::fclose(f);
    return v;
}
int failures = 0;
void check(bool ok, const std::string& what) {
    if (!ok && failures++ < 10) std::fprintf(stderr, "CHECK FAILED: %s\n", what.c_str());
}
uint32_t metaOf(const uint32_t* R, int j) { return (R[6 + (j >> 2)] >> (8 * (j & 3))) & 0xffu; }
bool internal(uint32_t meta) { return (meta & 0x18u) == 0x18u; }

struct Scene {
    std::vector<pt_object> objs;
    std::vector<int64_t> first, count, g0;   // per mesh; g0: its first shading index
    std::vector<pt_instance> inst;
    int64_t gTotal = 0;
};
struct Walk {
    const Scene& sc;
    const pt::InstancedTree& t;
    uint32_t slots;
    std::vector<int> seen;        // per (instance, shading index)
    std::vector<int> topVisits;   // per slot of the top level's region
    uint32_t maxTop = 0;
    size_t entries = 0;       // instance records reached
    int64_t steps = 0;
    double margin = 0.0;      // what an entry's planes keep around the world image below it
    int topDepth = 0;         // deepest node of the top level (root = 1; instance records not counted)

    const uint32_t* node(uint32_t s) const { return &t.nodes[(size_t)s * pt::kW8NodeDwords]; }

    // the primitives below a mesh-tree node whose slots must lie in [lo, hi)
    void collect(uint32_t s, uint32_t lo, uint32_t hi, std::vector<uint32_t>& out) {
        if (!(s >= lo && s < hi)) return check(false, "mesh-tree slot outside its mesh's relocated tree");
        if (++steps > (int64_t)1 << 26) return check(false, "walk does not end");
        const uint32_t* R = node(s);
        check(R[3] != pt::kW8InstanceFlag, "instance record inside a mesh tree");
        for (int j = 0; j < 8; j++) {
            const uint32_t m = metaOf(R, j);
            if (!m) continue;
            if (internal(m)) collect(R[4] + (m & 7u), lo, hi, out);
            else
                for (uint32_t q = 0; q < 3 && ((m >> 5) >> q & 1u); q++) out.push_back(R[5] + (m & 31u) + q);
        }
    }

    // an instance record at slot s, its box from its parent's planes
    void entry(uint32_t s, const double* lo, const double* hi) {
        const uint32_t* R = node(s);
        const uint32_t i = R[5];
        entries++;
        if (i >= sc.inst.size()) return check(false, "instance id in range");
        const pt_instance& I = sc.inst[i];
        const int mesh = I.mesh;
        check(R[2] == 0u && R[6] == 0u && R[7] == 0u, "dwords 2, 6, 7 of an instance record are zero");
        const uint32_t mlo = t.meshRoot[(size_t)mesh];
        const uint32_t mhi = (size_t)mesh + 1 < t.meshRoot.size() ? t.meshRoot[(size_t)mesh + 1] : slots;
        check(sc.count[(size_t)mesh] > 0, "an instance of an empty mesh is never reachable");
        check(R[4] >= mlo && R[4] < mhi, "dword 4 inside the relocated tree of the instance's mesh");
        check(std::memcmp(R + 8, &t.winst[(size_t)i * 16], 48) == 0, "record rows equal the winst rows");
        bool lin = true, still = true;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) lin = lin && I.m[4 * r + c] == (r == c ? 1.0f : 0.0f);
            still = still && I.m[4 * r + 3] == 0.0f;
        }
        check(R[0] == (lin && still ? 1u : 0u) && R[1] == (lin && !still ? 1u : 0u), "class dwords agree with the matrix");
        if (!(R[4] >= mlo && R[4] < mhi)) return;
        std::vector<uint32_t> below;
        collect(R[4], mlo, mhi, below);
        for (uint32_t p : below) {
            if ((size_t)(p + 1) * pt::kW8PrimDwords > t.prims.size()) { check(false, "primitive index in range"); continue; }
            const uint32_t* P = &t.prims[(size_t)p * pt::kW8PrimDwords];
            const int64_t g = P[3], k = g - sc.g0[(size_t)mesh];
            if (k < 0 || k >= sc.count[(size_t)mesh]) { check(false, "primitive belongs to the instance's mesh"); continue; }
            check(P[7] == (uint32_t)k, "record dword 7 is the object within its mesh");
            seen[(size_t)i * (size_t)sc.gTotal + (size_t)g]++;
            const pt_object& o = sc.objs[(size_t)(sc.first[(size_t)mesh] + k)];
            auto inside = [&](double x, double y, double z) {
                for (int a = 0; a < 3; a++) {
                    const double w = (double)I.m[4 * a] * x + (double)I.m[4 * a + 1] * y + (double)I.m[4 * a + 2] * z + (double)I.m[4 * a + 3];
                    if (!(lo[a] <= w - margin && w + margin <= hi[a])) return false;
                }
                return true;
            };
            bool ok = true;
            if (o.type == PT_SPHERE) {
                const double rr = std::fabs((double)o.v[3]);
                for (int c = 0; c < 8; c++)
                    ok = ok && inside(o.v[0] + ((c & 1) ? rr : -rr), o.v[1] + ((c & 2) ? rr : -rr), o.v[2] + ((c & 4) ? rr : -rr));
            } else {
                for (int v = 0; v < 3; v++) ok = ok && inside(o.v[3 * v], o.v[3 * v + 1], o.v[3 * v + 2]);
            }
            check(ok, "entry box contains the world image of the primitives below its sub-root");
        }
    }

    // a node of the top level: every child is internal (a node or an instance record)
    void top(uint32_t s, int level = 1) {
        const uint32_t* R = node(s);
        topDepth = level > topDepth ? level : topDepth;
        float p[3];
        std::memcpy(p, R, 12);
        for (int j = 0; j < 8; j++) {
            const uint32_t m = metaOf(R, j);
            if (!m) continue;
            if (!internal(m)) { check(false, "a leaf child in the top level"); continue; }
            const uint32_t c = R[4] + (m & 7u);
            if (c >= t.topCap) { check(false, "top-level slot inside the top level's region"); continue; }
            if (topVisits[c]++) { check(false, "top-level slot reached once"); continue; }
            maxTop = c > maxTop ? c : maxTop;
            double lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                const int e = (int)((R[3] >> (8 * a)) & 0xffu) - 127;
                const uint32_t ql = (R[8 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                const uint32_t qh = (R[10 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                lo[a] = (double)p[a] + std::ldexp((double)ql, e);
                hi[a] = (double)p[a] + std::ldexp((double)qh, e);
            }
            if (node(c)[3] == pt::kW8InstanceFlag) entry(c, lo, hi);
            else top(c, level + 1);
        }
    }
};

bool sameTree(const pt::InstancedTree& a, const pt::InstancedTree& b) {
    auto eq = [](const auto& x, const auto& y) {
        return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
    };
    return eq(a.nodes, b.nodes) && eq(a.prims, b.prims) && eq(a.shade, b.shade) && eq(a.winst, b.winst) && eq(a.reach, b.reach) &&
           eq(a.entries, b.entries) && eq(a.meshRoot, b.meshRoot) && eq(a.desc, b.desc) && eq(a.subBoxes, b.subBoxes) &&
           eq(a.entryPrims, b.entryPrims) && eq(a.entryRank, b.entryRank) && a.gBits == b.gBits && a.depth == b.depth &&
           a.maxDepthB == b.maxDepthB && a.topCap == b.topCap && std::memcmp(a.sceneCE, b.sceneCE, 16) == 0 &&
           std::memcmp(&a.mixLim, &b.mixLim, 4) == 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    Scene sc;
    sc.objs = readAll<pt_object>(argv[1]);
    const std::vector<int64_t> meshes = readAll<int64_t>(argv[2]);   // the firsts, then the counts
    sc.inst = readAll<pt_instance>(argv[3]);
    const std::vector<float> mats = readAll<float>(argv[4]);
    const int nm = (int)(meshes.size() / 2);
    sc.first.assign(meshes.begin(), meshes.begin() + nm);
    sc.count.assign(meshes.begin() + nm, meshes.end());
    for (int m = 0; m < nm; m++) { sc.g0.push_back(sc.gTotal); sc.gTotal += sc.count[(size_t)m]; }
    pt::InstancedIn in{};
    in.objs = sc.objs.data();
    in.meshFirst = sc.first.data();
    in.meshCount = sc.count.data();
    in.nMeshes = nm;
    in.inst = sc.inst.data();
    in.nInst = (int64_t)sc.inst.size();
    in.mats = mats.data();
    in.nmat = (int64_t)(mats.size() / 8);
    in.dynamic = std::atoi(argv[5]) != 0;
    in.rebraid = std::atoi(argv[6]);
    in.entryBudget = std::atoi(argv[7]);
    in.farExt = 2.0f;   // (the kernels' PT_INST_FAR_EXT)
    pt::InstancedTree t, again;
    const int rc = pt::buildInstancedTree(in, t);
    if (rc != PT_OK) {
        std::printf("rc %d: %s\n", rc, pt::lastError().c_str());
        return 3;
    }
    check(pt::buildInstancedTree(in, again) == PT_OK && sameTree(t, again), "two builds give byte-identical arrays");
    // downloaded arrays in place of the built ones
    const std::string mode = argc >= 13 ? argv[12] : "";
    int repDepth = t.depth;
    int64_t repSlots = (int64_t)(t.nodes.size() / pt::kW8NodeDwords);
    if (argc >= 13) {
        if (mode != "full" && mode != "top") return 2;
        const std::vector<uint32_t> dn = readAll<uint32_t>(argv[8]);
        const std::vector<float> dw = readAll<float>(argv[9]);
        repDepth = std::atoi(argv[10]);
        repSlots = std::atoll(argv[11]);
        check(dn.size() == t.nodes.size(), "downloaded node array has the layout's size");
        check(repSlots == (int64_t)(t.nodes.size() / pt::kW8NodeDwords), "reported slots are the layout's");
        check(dw.size() == t.winst.size() && std::memcmp(dw.data(), t.winst.data(), dw.size() * 4) == 0,
              "downloaded instance rows equal the host's rows for these matrices");
        if (mode == "full")
            check(dn.size() == t.nodes.size() && std::memcmp(dn.data(), t.nodes.data(), dn.size() * 4) == 0,
                  "downloaded nodes equal the host build's");
        if (failures) {
            std::printf("slots %zu top %u failures %d\n", t.nodes.size() / pt::kW8NodeDwords, t.topCap, failures);
            return 1;
        }
        t.nodes = dn;
        t.winst = dw;
    }

    const size_t ni = sc.inst.size();
    const uint32_t slots = (uint32_t)(t.nodes.size() / pt::kW8NodeDwords);
    check(t.nodes.size() % pt::kW8NodeDwords == 0 && t.nodes.size() / pt::kW8NodeDwords < ((size_t)1 << 24), "fewer than 2^24 node slots");
    int gBits = 1;
    while (((int64_t)1 << gBits) < sc.gTotal) gBits++;
    check(t.gBits == gBits, "gBits is the smallest with 2^gBits >= the mesh primitives");
    check(pt::wideStackFor(t.depth) >= 0, "wideStackFor(depth) >= 0");
    check(t.meshRoot.size() == (size_t)nm && t.winst.size() >= ni * 16, "array sizes");
    check(t.topCap >= 1 && t.topCap <= slots && nm > 0 && t.meshRoot[0] == t.topCap, "the mesh trees start behind the top level's region");
    for (int m = 0; m + 1 < nm; m++) check(t.meshRoot[(size_t)m] <= t.meshRoot[(size_t)m + 1], "mesh trees in mesh order");

    Walk w{sc, t, slots, std::vector<int>(ni * (size_t)sc.gTotal, 0), std::vector<int>(t.topCap, 0)};
    // The top level's own margin: 2^emin of its root box (buildWide8Leaf; wideWriteKernel's rule on
    // the device).  The root box is the union of the entries' boxes, which contain the world image
    // of the primitives, so the extent taken from that image in fp64 is never larger than the
    // builder's and this margin never more than the one the builder kept.
    {
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < ni; i++) {
            const pt_instance& I = sc.inst[i];
            for (int64_t k = 0; k < sc.count[(size_t)I.mesh]; k++) {
                const pt_object& o = sc.objs[(size_t)(sc.first[(size_t)I.mesh] + k)];
                auto grow = [&](double x, double y, double z) {
                    for (int a = 0; a < 3; a++) {
                        const double v = (double)I.m[4 * a] * x + (double)I.m[4 * a + 1] * y + (double)I.m[4 * a + 2] * z + (double)I.m[4 * a + 3];
                        mn[a] = std::fmin(mn[a], v);
                        mx[a] = std::fmax(mx[a], v);
                    }
                };
                if (o.type == PT_SPHERE) {
                    const double rr = std::fabs((double)o.v[3]);
                    for (int c = 0; c < 8; c++) grow(o.v[0] + ((c & 1) ? rr : -rr), o.v[1] + ((c & 2) ? rr : -rr), o.v[2] + ((c & 4) ? rr : -rr));
                } else {
                    for (int v = 0; v < 3; v++) grow(o.v[3 * v], o.v[3 * v + 1], o.v[3 * v + 2]);
                }
            }
        }
        double ext = 0.0;
        for (int a = 0; a < 3; a++) ext = std::fmax(ext, std::fmax(std::fmax(std::fabs(mn[a]), std::fabs(mx[a])), mx[a] - mn[a]));
        const int emin = ext > 0.0 && std::isfinite(ext) ? std::max(-100, (int)std::ceil(std::log2(ext)) - pt::kW8EminShift) : -100;
        w.margin = std::ldexp(1.0, emin);
    }
    check(w.node(0)[3] != pt::kW8InstanceFlag, "slot 0 is a node");
    w.top(0);
    check(repDepth == w.topDepth + 1 + t.maxDepthB + 1, "reported depth is the walk's: top levels, the marker, the deepest mesh tree");
    check(pt::wideStackFor(repDepth) >= 0, "wideStackFor(reported depth) >= 0");
    check(w.entries == t.entries.size(), "one instance record per entry");
    for (size_t i = 0; i < ni; i++) {
        const int mesh = sc.inst[i].mesh;
        for (int64_t g = 0; g < sc.gTotal; g++) {
            const bool mine = g >= sc.g0[(size_t)mesh] && g < sc.g0[(size_t)mesh] + sc.count[(size_t)mesh];
            check(w.seen[i * (size_t)sc.gTotal + (size_t)g] == (mine ? 1 : 0), "every (instance, mesh primitive) pair reachable exactly once");
        }
    }
    // every instance record of the array, reachable or not
    for (uint32_t s = 0; s < t.topCap; s++) {
        const uint32_t* R = w.node(s);
        if (w.topVisits[s] && s > 0 && R[5] < ni && R[3] == pt::kW8InstanceFlag) continue;   // (checked in the walk)
        check(R[3] != pt::kW8InstanceFlag, "an instance record nobody reaches");
    }
    uint32_t objBase = 0;
    for (size_t i = 0; i < ni; i++) {
        uint32_t ob;
        std::memcpy(&ob, &t.winst[i * 16 + 12], 4);
        check(ob == objBase, "winst objBase");
        objBase += (uint32_t)sc.count[(size_t)sc.inst[i].mesh];
    }
    if (in.dynamic) {
        check((int64_t)t.topCap == pt::instanceTopSlots((int64_t)t.entries.size()), "topCap == instanceTopSlots(entries)");
        int64_t e = 0;
        for (const pt::InstBoxDesc& D : t.desc) e += D.entryCount;
        check(t.desc.size() == ni && e == (int64_t)t.entries.size(), "desc entry counts sum to the entries");
        check(t.entryRank.size() == t.entries.size() && t.entryPrims.size() == t.entries.size() * pt::kW8PrimDwords, "entry record sizes");
    } else {
        check(w.maxTop + 8 >= t.topCap || t.topCap == 1, "the mesh trees start right behind the top level");
    }
    std::printf("slots %u top %u entries %zu depth %d gBits %d failures %d\n", slots, t.topCap, t.entries.size(), t.depth, t.gBits,
                failures);
    return failures ? 1 : 0;
}
