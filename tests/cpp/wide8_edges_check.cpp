// CPU check of the edge-form triangle records (host/pt_wide8.hpp edgeTriRecords) the wide render
// kernels' LEAF step reads (TEST INFRASTRUCTURE: compiled and run by tests/test_wide_edges.py; the
// product never uses it).
//   1. objects.bin -> the leaf-order records, reference ranks and wide tree exactly as libpt builds
//      them (as tests/cpp/wide8_check.cpp), then the conversion of the tree's records;
//   2. hand-made records: edges that are denormal, that cancel to +0 and to -0, against expected bits.
// Every e1 / e2 word must be the fp32 subtraction of the vertex words, bit for bit; v0 and word 3 of
// each 16-B word are unchanged; the records keep their count and order.
// usage: wide8_edges_check objects.bin
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt.h"
#include "pt_wide8.hpp"

extern "C" {
typedef struct { int32_t left, right, parent, objid; float bmin[3], bmax[3]; } orc_node;
int orc_morton_keys(const pt_object* objs, int64_t n, int include_origin, uint64_t* keys_out);
int orc_build_lbvh(const pt_object* objs, int64_t n, const uint64_t* keys, int tight, orc_node* nodes);
}

namespace {
int failures = 0;
void check(bool ok, const std::string& what) {
    if (!ok && failures++ < 10) std::fprintf(stderr, "CHECK FAILED: %s\n", what.c_str());
}
// one fp32 subtraction of two words, kept out of the optimiser's sight
uint32_t subBits(uint32_t a, uint32_t b) {
    volatile float x, y, r;
    float fa, fb;
    std::memcpy(&fa, &a, 4);
    std::memcpy(&fb, &b, 4);
    x = fa;
    y = fb;
    r = x - y;
    const float out = r;
    uint32_t u;
    std::memcpy(&u, &out, 4);
    return u;
}
// the conversion of `recs` (n records) checked word for word; returns the converted records
std::vector<uint32_t> convertChecked(const std::vector<uint32_t>& recs, const char* what) {
    const int64_t n = (int64_t)(recs.size() / pt::kW8PrimDwords);
    std::vector<uint32_t> out(recs.size() + 4, 0xdeadbeefu);   // (4 guard words behind the records)
    pt::edgeTriRecords(recs.data(), n, out.data());
    for (int g = 0; g < 4; g++) check(out[recs.size() + g] == 0xdeadbeefu, std::string(what) + ": writes past the last record");
    out.resize(recs.size());
    for (int64_t k = 0; k < n; k++) {
        const uint32_t* s = &recs[(size_t)k * 12];
        const uint32_t* d = &out[(size_t)k * 12];
        for (int a = 0; a < 3; a++) {
            check(d[a] == s[a], std::string(what) + ": v0 unchanged");
            check(d[4 + a] == subBits(s[4 + a], s[a]), std::string(what) + ": e1 = v1 - v0");
            check(d[8 + a] == subBits(s[8 + a], s[a]), std::string(what) + ": e2 = v2 - v0");
        }
        check(d[3] == s[3], std::string(what) + ": rank unchanged");
        check(d[7] == s[7] && d[11] == s[11], std::string(what) + ": words 7 and 11 unchanged");
    }
    return out;
}
template <class T>
std::vector<T> readAll(const char* path) {
    std::vector<T> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
    std::fclose(f);
    return v;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::vector<pt_object> objs = readAll<pt_object>(argv[1]);
    const int64_t n = (int64_t)objs.size();
    if (n < 1) return 2;
    std::vector<uint64_t> keys((size_t)n);
    orc_morton_keys(objs.data(), n, 1, keys.data());
    std::vector<orc_node> nd((size_t)(2 * n - 1));
    orc_build_lbvh(objs.data(), n, keys.data(), 1, nd.data());
    // leaf-order primitive records and boxes, as the device's leafGatherKernel writes them
    std::vector<uint32_t> prims((size_t)n * 12, 0u);
    std::vector<float> boxes((size_t)n * 6);
    for (int64_t k = 0; k < n; k++) {
        const pt_object& o = objs[keys[k] & 0xffffffffu];
        if (o.type == PT_SPHERE) {
            std::fprintf(stderr, "triangle-only scenes have edge records; object %lld is a sphere\n", (long long)k);
            return 2;
        }
        pt::primRecord(o, (uint32_t)(keys[k] & 0xffffffffu), &prims[(size_t)k * 12], &boxes[(size_t)k * 6]);
    }
    std::vector<uint32_t> lref((size_t)std::max<int64_t>(1, n - 1)), rref(lref.size());
    for (int64_t i = 0; i + 1 < n; i++) {
        auto ref = [&](int32_t c) { return c >= n - 1 ? (0x80000000u | (uint32_t)(c - (n - 1))) : (uint32_t)c; };
        lref[(size_t)i] = ref(nd[(size_t)i].left);
        rref[(size_t)i] = ref(nd[(size_t)i].right);
    }
    const std::vector<uint32_t> rank = pt::referenceRanks(lref.data(), rref.data(), 1, n);
    pt::Wide8 w;
    std::string err;
    if (!pt::buildWide8(prims.data(), boxes.data(), rank.data(), n, w, err)) {
        std::fprintf(stderr, "build failed: %s\n", err.c_str());
        return 1;
    }
    check((int64_t)(w.prims.size() / pt::kW8PrimDwords) == n, "one wide-order record per primitive");
    const std::vector<uint32_t> e = convertChecked(w.prims, "scene");
    check(e.size() == w.prims.size(), "record count");
    // the order is the tree's: record i keeps the rank of record i (checked above), every rank once
    std::vector<int> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; i++)
        if (e[(size_t)i * 12 + 3] < (uint32_t)n) seen[e[(size_t)i * 12 + 3]]++;
    for (int64_t k = 0; k < n; k++) check(seen[(size_t)k] == 1, "every rank exactly once");
    int64_t nonzero = 0;
    for (int64_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) nonzero += (e[(size_t)i * 12 + 4 + a] << 1) != 0u;
    check(nonzero > n, "the scene's edges are not all zero");

    // 2. hand-made records {v0, rank}{v1, obj}{v2, 0}: expected edge words written out
    struct Case { uint32_t v0, v1, v2, e1, e2; const char* what; };
    const Case cases[] = {
        {0x00800000u, 0x00800001u, 0x00800003u, 0x00000001u, 0x00000003u, "normal vertices, denormal edges (no flush to zero)"},
        {0x80800000u, 0x80800001u, 0x007fffffu, 0x80000001u, 0x00ffffffu, "negative denormal edge; denormal minus normal"},
        {0x00000005u, 0x00000002u, 0x00000009u, 0x80000003u, 0x00000004u, "denormal vertices"},
        {0x3f800000u, 0x3f800000u, 0x3f800000u, 0x00000000u, 0x00000000u, "equal vertices cancel to +0"},
        {0x00000000u, 0x80000000u, 0x00000000u, 0x80000000u, 0x00000000u, "-0 minus +0 is -0; +0 minus +0 is +0"},
        {0x80000000u, 0x80000000u, 0x00000000u, 0x00000000u, 0x00000000u, "-0 minus -0 and +0 minus -0 are +0"},
        {0x43c80000u, 0x43c80001u, 0xc3c80000u, 0x38000000u, 0xc4480000u, "one ulp at 400; 400 mirrored"},
    };
    const int nc = (int)(sizeof(cases) / sizeof(cases[0]));
    std::vector<uint32_t> hand((size_t)nc * 12);
    for (int i = 0; i < nc; i++) {
        uint32_t* r = &hand[(size_t)i * 12];
        for (int a = 0; a < 3; a++) { r[a] = cases[i].v0; r[4 + a] = cases[i].v1; r[8 + a] = cases[i].v2; }
        r[3] = 0x3fffff00u + (uint32_t)i;   // (a rank: any word, copied)
        r[7] = 0x12345678u;
        r[11] = 0u;
    }
    const std::vector<uint32_t> he = convertChecked(hand, "hand-made");
    for (int i = 0; i < nc; i++)
        for (int a = 0; a < 3; a++) {
            check(he[(size_t)i * 12 + 4 + a] == cases[i].e1, std::string("e1 bits: ") + cases[i].what);
            check(he[(size_t)i * 12 + 8 + a] == cases[i].e2, std::string("e2 bits: ") + cases[i].what);
        }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("%lld scene records, %d hand-made records ok\n", (long long)n, nc);
    return 0;
}
