// CPU check of the wide render kernels' deferred leaf-box rule (TEST INFRASTRUCTURE: compiled and
// run by tests/test_wide_deferred_rule.py; the product never uses it).  Triangle-only scenes.
// Builds the binary LBVH with the oracle (oracle/), the reference ranks, the wide tree and the
// per-rank exact boxes exactly as libpt does, then traces every ray through scalar restatements of
//   new: renderKernelWF<.., WIDE>'s loop as wideTestTri runs it (plain minimum of (t, rank), t2 = the
//        second-smallest candidate distance) and the SHADE step's deferredRedo on the final hit's
//        box (pt_device.hip);
//   old: the per-candidate rule of wideTest<false> (box test, take, window, sticky redo), which the
//        sphere scenes and the ray-query kernels keep.
// Writes {leaf k or -1, t, redo} of the new rule, then of the old rule, per ray.
// usage: wide8_deferred_check objects.bin rays.bin out.bin
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
float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
struct V { float x, y, z; };
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V cross(V u, V v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
const uint32_t* P;     // wide-order primitive records
const uint32_t* N;     // wide nodes
const float* B;        // exact boxes by rank (pt::exactTriBox)

// primHitAny (pt_device.hip) for a triangle: the reference's test (cuda_object.h:69-92) without
// the closest-hit bound
float primT(int i, V o, V d, float tmin) {
    const uint32_t* r = P + 12 * i;
    V v0{u2f(r[0]), u2f(r[1]), u2f(r[2])}, v1{u2f(r[4]), u2f(r[5]), u2f(r[6])}, v2{u2f(r[8]), u2f(r[9]), u2f(r[10])};
    V e1 = sub(v1, v0), e2 = sub(v2, v0), s1 = cross(d, e2);
    const float det = dot(s1, e1);
    if (det == 0) return -1;
    V s = sub(o, v0), s2 = cross(s, e1);
    const float inv = 1.0f / det, t = dot(s2, e2) * inv, b1 = dot(s1, s) * inv, b2 = dot(s2, d) * inv;
    if (b1 >= 1 || b1 <= 0 || b2 >= 1 || b2 <= 0 || b1 + b2 >= 1 || t <= tmin) return -1;
    return t;
}
// slabPair (pt_device.hip) on {mn, mx} pairs per axis with tmax = +inf: {passes, entry lo}
bool slab(const float* box, V o, V inv, float tmin, float& lo) {
    const float ov[3] = {o.x, o.y, o.z}, iv[3] = {inv.x, inv.y, inv.z};
    float l = tmin, h = INFINITY;
    for (int a = 0; a < 3; a++) {
        float t0 = (box[2 * a] - ov[a]) * iv[a], t1 = (box[2 * a + 1] - ov[a]) * iv[a];
        if (iv[a] < 0) std::swap(t0, t1);
        l = std::fmax(l, t0);   // (fmaxf / fminf drop a NaN, as v_max_f32 / v_min_f32)
        h = std::fmin(h, t1);
    }
    lo = l;
    return !(h < l);
}
// the old rule's box: from the record's vertices (refLeafBox)
bool leafBox(int i, V o, V inv, float tmin, float& lo) {
    float box[pt::kW8BoxFloats];
    pt::exactTriBox(reinterpret_cast<const float*>(P + 12 * i), box);
    return slab(box, o, inv, tmin, lo);
}
float med3(float a, float b, float c) { return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c)); }

// renderKernelWF<.., WIDE>'s traversal for one ray; returns the best rank (-1), sets redo
int traceWide(V o, V d, float tmin, float& closest, bool single, bool deferred, bool& redo) {
    const V inv{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    const uint32_t oct = (inv.x < 0 ? 1u : 0u) | (inv.y < 0 ? 2u : 0u) | (inv.z < 0 ? 4u : 0u);
    uint32_t ng = 1u << oct, tgBase = 0, tg = 0, stk[64];
    int sp = 0, best = -1;
    float bestLo = deferred ? INFINITY : -INFINITY;   // deferred: t2
    closest = INFINITY;
    redo = false;
    for (;;) {
        while (tg) {
            const int i = (int)(tgBase + (uint32_t)__builtin_ctz(tg));
            tg &= tg - 1u;
            const float t = primT(i, o, d, tmin);
            if (!(t >= 0)) continue;
            const int k = (int)P[12 * i + 3];
            if (deferred) {   // wideTestTri
                const bool better = t < closest || (t == closest && k < best);
                bestLo = med3(t, closest, bestLo);
                if (better) { closest = t; best = k; }
                continue;
            }
            const bool tie = best >= 0 && k < best;   // wideTest<false>
            if (t >= closest && t < bestLo) redo = true;
            if (t < closest || (t == closest && tie)) {
                bool take = true;
                float lo2 = -INFINITY;
                if (!single) {
                    float lo;
                    const bool h = leafBox(i, o, inv, tmin, lo);
                    take = h && !(closest < lo);
                    if (h && closest < lo) redo = true;
                    if (t < lo) lo2 = lo;
                }
                if (take) { closest = t; best = k; bestLo = lo2; }
            }
        }
        if ((ng & 0xffu) == 0) {
            if (sp == 0) break;
            ng = stk[--sp];
        }
        const uint32_t bit = (uint32_t)__builtin_ctz(ng & 0xffu);
        const uint32_t child = (ng >> 8) + (bit ^ oct);
        ng &= ~(1u << bit);
        if (ng & 0xffu) stk[sp++] = ng;
        const uint32_t* R = N + 20 * child;
        float a[3], b[3];
        const float ov[3] = {o.x, o.y, o.z}, iv[3] = {inv.x, inv.y, inv.z};
        for (int ax = 0; ax < 3; ax++) {
            a[ax] = u2f(((R[3] >> (8 * ax)) & 0xffu) << 23) * iv[ax];
            b[ax] = (u2f(R[ax]) - ov[ax]) * iv[ax];
        }
        uint32_t hits = 0;
        for (int j = 0; j < 8; j++) {
            const uint32_t meta = ((j < 4 ? R[6] : R[7]) >> (8 * (j & 3))) & 0xffu;
            float lo = tmin, hi = closest;
            for (int ax = 0; ax < 3; ax++) {
                const uint32_t ql = (R[8 + 4 * ax + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                const uint32_t qh = (R[10 + 4 * ax + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                const uint32_t qn = iv[ax] < 0 ? qh : ql, qf = iv[ax] < 0 ? ql : qh;
                lo = std::fmax(lo, std::fma((float)qn, a[ax], b[ax]));
                hi = std::fmin(hi, std::fma((float)qf, a[ax], b[ax]));
            }
            if (lo <= hi && meta) {
                uint32_t bi = meta & 31u;
                if ((meta & 0x18u) == 0x18u) bi = 24u + ((bi - 24u) ^ oct);
                hits |= (meta >> 5) << bi;
            }
        }
        ng = (R[4] << 8) | (hits >> 24);
        tgBase = R[5];
        tg = hits & 0xffffffu;
    }
    if (deferred && !single && best >= 0) {   // SHADE: deferredRedo on the final hit's box
        float lo;
        const bool h = slab(B + (size_t)best * pt::kW8BoxFloats, o, inv, tmin, lo);
        redo = !h || (closest < lo && bestLo < lo);
    }
    return best;
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
    if (argc < 4) return 2;
    const std::vector<pt_object> objs = readAll<pt_object>(argv[1]);
    const std::vector<float> rays = readAll<float>(argv[2]);
    const int64_t n = (int64_t)objs.size(), nr = (int64_t)rays.size() / 6;
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
            std::fprintf(stderr, "triangle-only scenes\n");
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
    // the per-rank exact boxes, as buildWide (pt_device.hip) fills DevScene::wbox
    std::vector<float> wbox((size_t)n * pt::kW8BoxFloats);
    for (int64_t k = 0; k < n; k++)
        pt::exactTriBox(reinterpret_cast<const float*>(&prims[(size_t)k * 12]), &wbox[(size_t)rank[k] * pt::kW8BoxFloats]);
    pt::Wide8 w;
    std::string err;
    if (!pt::buildWide8(prims.data(), boxes.data(), rank.data(), n, w, err)) {
        std::fprintf(stderr, "build failed: %s\n", err.c_str());
        return 1;
    }
    P = w.prims.data();
    N = w.nodes.data();
    B = wbox.data();
    std::vector<int> kOfRank((size_t)n, -1);
    for (int64_t k = 0; k < n; k++) kOfRank[rank[k]] = (int)k;
    std::vector<float> out((size_t)nr * 6);
    for (int64_t i = 0; i < nr; i++) {
        const float* r = &rays[(size_t)i * 6];
        for (int old = 0; old < 2; old++) {
            float t = 0;
            bool redo = false;
            const int b = traceWide(V{r[0], r[1], r[2]}, V{r[3], r[4], r[5]}, 0.001f, t, n == 1, old == 0, redo);
            out[(size_t)i * 6 + 3 * old + 0] = (float)(b < 0 ? -1 : kOfRank[(size_t)b]);
            out[(size_t)i * 6 + 3 * old + 1] = t;
            out[(size_t)i * 6 + 3 * old + 2] = redo ? 1.0f : 0.0f;
        }
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    return 0;
}
