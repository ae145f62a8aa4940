// pt_instancing.cpp — host build of an instanced scene's two-level tree (see pt_instancing.hpp).
#include "pt_instancing.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "pt_error.hpp"

namespace pt {

int wideStackFor(int depth) {
    for (int st : {8, 16, 24})
        if (depth <= st) return st;
    return -1;
}

float mixLimit(double m) {
    if (!(m > 0.0) || !std::isfinite(m)) return m == 0.0 ? FLT_MAX : -1.0f;
    int ex = 0;
    const double f = std::frexp(m, &ex);   // m = f * 2^ex, f in [0.5, 1): ceil(log2(m)) = ex, or ex - 1 at f = 0.5
    const int eS = (f == 0.5 ? ex - 1 : ex) + 1;
    if (eS > 100) return -1.0f;
    if (103 - eS >= 127) return FLT_MAX;
    return std::ldexp(1.0f, 103 - eS);
}

namespace {
uint32_t instanceOfRecord(const uint32_t* rec) { return rec[7]; }
}  // namespace

void writeInstanceRecord(uint32_t e, uint32_t* dst, void* ctx) {
    const InstRecCtx& c = *static_cast<const InstRecCtx*>(ctx);
    const InstEntry& E = (*c.entries)[e];
    std::memset(dst, 0, kW8NodeDwords * 4);
    dst[0] = (*c.ident)[E.inst] == 1 ? 1u : 0u;
    dst[1] = (*c.ident)[E.inst] == 2 ? 1u : 0u;   // translation only: the kernels move the origin, keep the direction
    dst[3] = kW8InstanceFlag;
    dst[4] = E.slot;   // (+ the mesh tree's base slot once the layout is known)
    dst[5] = E.inst;
    dst[6] = E.mesh;   // (layout only; cleared with the relocation)
    std::memcpy(dst + 8, (*c.minv)[E.inst].data(), 48);
}

std::vector<SubRoot> nodeChildren(const Wide8& w, uint32_t slot) {
    std::vector<SubRoot> out;
    if (w.nodes.size() < (size_t)(slot + 1) * kW8NodeDwords) return out;
    const uint32_t* R = w.nodes.data() + (size_t)slot * kW8NodeDwords;
    float p[3];
    std::memcpy(p, R, 12);
    for (int j = 0; j < 8; j++) {
        const uint32_t mb = (R[6 + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
        if (mb == 0u) continue;
        if ((mb & 0xf8u) != 0x38u) return {};   // a leaf child at the root
        SubRoot sr;
        sr.slot = R[4] + (mb & 7u);
        for (int a = 0; a < 3; a++) {
            const int e = (int)((R[3] >> (8 * a)) & 0xffu) - 127;
            const uint32_t ql = (R[8 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
            const uint32_t qh = (R[10 + 4 * a + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
            sr.box[a] = (double)p[a] + std::ldexp((double)ql, e);
            sr.box[3 + a] = (double)p[a] + std::ldexp((double)qh, e);
        }
        out.push_back(sr);
    }
    return out;
}

void meshSubRoots(const Wide8& w, uint32_t slot, const double* box, int levels, std::vector<SubRoot>& out) {
    std::vector<SubRoot> ch = levels > 0 ? nodeChildren(w, slot) : std::vector<SubRoot>{};
    if (ch.empty()) {
        SubRoot sr;
        sr.slot = slot;
        for (int k = 0; k < 6; k++) sr.box[k] = box[k];
        out.push_back(sr);
        return;
    }
    for (const SubRoot& c : ch) meshSubRoots(w, c.slot, c.box, levels - 1, out);
}

void meshSubRootsBudget(const Wide8& w, size_t budget, std::vector<SubRoot>& out) {
    out = nodeChildren(w, 0u);
    if (out.empty()) return;
    auto area = [](const SubRoot& r) {
        const double x = r.box[3] - r.box[0], y = r.box[4] - r.box[1], z = r.box[5] - r.box[2];
        return x * y + y * z + z * x;
    };
    std::vector<bool> closed(out.size(), false);
    for (;;) {
        int pick = -1;
        double best = -1.0;
        for (size_t i = 0; i < out.size(); i++)
            if (!closed[i] && area(out[i]) > best) { best = area(out[i]); pick = (int)i; }
        if (pick < 0) break;
        std::vector<SubRoot> ch = nodeChildren(w, out[(size_t)pick].slot);
        if (ch.empty() || out.size() - 1 + ch.size() > budget) { closed[(size_t)pick] = true; continue; }
        out.erase(out.begin() + pick);
        closed.erase(closed.begin() + pick);
        for (const SubRoot& c : ch) { out.push_back(c); closed.push_back(false); }
    }
}

bool instanceInverse(const pt_instance& I, std::array<float, 12>& minv, std::array<double, 12>& w2o, uint8_t& cls) {
    const double a[3][3] = {{I.m[0], I.m[1], I.m[2]}, {I.m[4], I.m[5], I.m[6]}, {I.m[8], I.m[9], I.m[10]}};
    const double t[3] = {I.m[3], I.m[7], I.m[11]};
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(std::fabs(det) > 1e-30) || !std::isfinite(det)) return false;
    double inv[3][3];
    inv[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det;
    inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    inv[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det;
    inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    inv[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det;
    inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    bool id = true, lin = true;
    for (int r = 0; r < 3; r++) {
        const double it = -(inv[r][0] * t[0] + inv[r][1] * t[1] + inv[r][2] * t[2]);
        for (int c = 0; c < 3; c++) {
            minv[(size_t)(4 * r + c)] = (float)inv[r][c];
            lin = lin && a[r][c] == (r == c ? 1.0 : 0.0);
        }
        minv[(size_t)(4 * r + 3)] = (float)it;
        for (int c = 0; c < 3; c++) w2o[(size_t)(4 * r + c)] = inv[r][c];
        w2o[(size_t)(4 * r + 3)] = it;
        id = id && t[r] == 0.0;
    }
    id = id && lin;
    cls = id ? 1 : (lin ? 2 : 0);
    return true;
}

int instanceRecords(const InstancedIn& in, InstRecords& R) {
    const int64_t ni = in.nInst;
    R.minv.resize((size_t)ni);
    R.ident.assign((size_t)ni, 0);
    R.winst.assign((size_t)std::max<int64_t>(1, ni) * 16, 0.0f);
    R.w2o.resize((size_t)ni);
    uint32_t objBase = 0;
    for (int64_t i = 0; i < ni; i++) {
        const pt_instance& I = in.inst[(size_t)i];
        if (!instanceInverse(I, R.minv[(size_t)i], R.w2o[(size_t)i], R.ident[(size_t)i]))
            return fail(PT_ERR_INVALID, "instanced scene: instance " + std::to_string(i) + " has a singular transform");
        for (int k = 0; k < 12; k++) R.winst[(size_t)i * 16 + (size_t)k] = R.minv[(size_t)i][(size_t)k];
        const uint32_t ob = objBase, idf = R.ident[(size_t)i];   // identity | translation only
        std::memcpy(&R.winst[(size_t)i * 16 + 12], &ob, 4);
        std::memcpy(&R.winst[(size_t)i * 16 + 13], &idf, 4);
        objBase += (uint32_t)in.meshCount[(size_t)I.mesh];
    }
    return PT_OK;
}

void instanceScalars(const InstancedIn& in, const double* wmn, const double* wmx, const std::vector<std::array<double, 12>>& w2o,
                     InstScalars& out, std::vector<double>& reach) {
    const int64_t ni = in.nInst;
    double wext = 0.0, wm = 0.0;
    for (int a = 0; a < 3; a++) {
        out.ce[a] = (float)(0.5 * (wmn[a] + wmx[a]));
        wext = std::max(wext, wmx[a] - wmn[a]);
        wm = std::max({wm, std::fabs(wmn[a]), std::fabs(wmx[a]), wmx[a] - wmn[a]});
    }
    out.ce[3] = std::nextafter((float)wext, INFINITY);
    out.mixLim = mixLimit(wm);
    reach.assign((size_t)in.nMeshes, 0.0);
    for (int64_t i = 0; i < ni; i++) {
        const std::array<double, 12>& W = w2o[(size_t)i];
        double r = 0.0;
        for (int c = 0; c < 8; c++) {   // corners of the cube of half-size farExt world extents (+ 1 %)
            const double h = 1.01 * in.farExt * wext;
            const double p[3] = {0.5 * (wmn[0] + wmx[0]) + ((c & 1) ? h : -h), 0.5 * (wmn[1] + wmx[1]) + ((c & 2) ? h : -h),
                                 0.5 * (wmn[2] + wmx[2]) + ((c & 4) ? h : -h)};
            for (int a = 0; a < 3; a++)
                r = std::max(r, std::fabs(W[(size_t)(4 * a)] * p[0] + W[(size_t)(4 * a + 1)] * p[1] +
                                          W[(size_t)(4 * a + 2)] * p[2] + W[(size_t)(4 * a + 3)]));
        }
        const int m = in.inst[(size_t)i].mesh;
        reach[(size_t)m] = std::max(reach[(size_t)m], r);
    }
}

bool instanceTop(const InstRecords& rec, const std::vector<InstEntry>& entries, const float* eboxes, Wide8& top, std::string& err) {
    std::vector<uint32_t> iprims(entries.size() * kW8PrimDwords, 0u);
    for (size_t e = 0; e < entries.size(); e++) iprims[e * kW8PrimDwords + 7] = (uint32_t)e;
    if (!buildWide8Leaf(iprims.data(), eboxes, nullptr, (int64_t)entries.size(), 1, top, err)) return false;
    InstRecCtx ctx{&rec.minv, &rec.ident, &entries};
    return instanceLeaves(top, instanceOfRecord, writeInstanceRecord, &ctx, err);
}

int64_t instanceTopSlots(int64_t n) { return 1 + 8 * std::max<int64_t>(1, n - 1); }

namespace {
// The 48-byte shading record of mesh primitive k (object space): the triangle's normal or the
// sphere's {centre, radius}, then the object's material inline, as the LBVH's leafGatherKernel
// writes it: {albedo, fuzz}, {ir, type | sphere << 16, mat, k}.
void meshShadeRecord(const pt_object& o, uint32_t k, const float* mats, uint32_t* sh) {
    float shf[12] = {};
    if (o.type == PT_SPHERE) {
        shf[0] = o.v[0]; shf[1] = o.v[1]; shf[2] = o.v[2]; shf[3] = o.v[3];
    } else {
        // triangle.h:17-19 normalize(cross(v1 - v0, v2 - v0)), the device's operation order
        const float e1[3] = {o.v[3] - o.v[0], o.v[4] - o.v[1], o.v[5] - o.v[2]};
        const float e2[3] = {o.v[6] - o.v[0], o.v[7] - o.v[1], o.v[8] - o.v[2]};
        const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float l = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (l != 0.0f) {
            const float il = 1.0f / l;
            for (int a = 0; a < 3; a++) shf[a] = il * c[a];
        }
    }
    const float* m = mats + (size_t)o.mat * 8;
    for (int a = 0; a < 5; a++) shf[4 + a] = m[a];
    std::memcpy(sh, shf, sizeof(shf));
    uint32_t tp;
    std::memcpy(&tp, &m[5], 4);
    sh[9] = tp | (o.type == PT_SPHERE ? 0x10000u : 0u);
    sh[10] = (uint32_t)o.mat;
    sh[11] = k;
}

// The exact world box of instance I of the objects [objs, objs + n): every vertex (a sphere: the
// eight corners of its box) through the matrix in double.  Also grows the world box wmn / wmx.
void instanceWorldBox(const pt_instance& I, const pt_object* objs, int64_t n, double* box, double* wmn, double* wmx) {
    const double a[3][3] = {{I.m[0], I.m[1], I.m[2]}, {I.m[4], I.m[5], I.m[6]}, {I.m[8], I.m[9], I.m[10]}};
    const double t[3] = {I.m[3], I.m[7], I.m[11]};
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto grow = [&](double x, double y, double z) {
        const double p[3] = {x, y, z};
        for (int r = 0; r < 3; r++) {
            const double w = a[r][0] * p[0] + a[r][1] * p[1] + a[r][2] * p[2] + t[r];
            mn[r] = std::min(mn[r], w);
            mx[r] = std::max(mx[r], w);
        }
    };
    for (int64_t k = 0; k < n; k++) {
        const pt_object& o = objs[k];
        if (o.type == PT_SPHERE) {
            const double rr = std::fabs((double)o.v[3]);
            for (int c = 0; c < 8; c++)
                grow(o.v[0] + ((c & 1) ? rr : -rr), o.v[1] + ((c & 2) ? rr : -rr), o.v[2] + ((c & 4) ? rr : -rr));
        } else {
            for (int v = 0; v < 3; v++) grow(o.v[3 * v], o.v[3 * v + 1], o.v[3 * v + 2]);
        }
    }
    for (int r = 0; r < 3; r++) { wmn[r] = std::min(wmn[r], mn[r]); wmx[r] = std::max(wmx[r], mx[r]); }
    for (int r = 0; r < 3; r++) {
        box[r] = mn[r];
        box[3 + r] = mx[r];
    }
}

// The world box of sub-root box `sb` under instance I (8 corners in double), never beyond the
// instance's exact box.
void subRootWorldBox(const pt_instance& I, const double* sb, const double* ibox, double* b) {
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int c = 0; c < 8; c++) {
        const double q[3] = {sb[(c & 1) ? 3 : 0], sb[(c & 2) ? 4 : 1], sb[(c & 4) ? 5 : 2]};
        for (int a = 0; a < 3; a++) {
            const double w = (double)I.m[4 * a] * q[0] + (double)I.m[4 * a + 1] * q[1] + (double)I.m[4 * a + 2] * q[2] +
                             (double)I.m[4 * a + 3];
            mn[a] = std::min(mn[a], w);
            mx[a] = std::max(mx[a], w);
        }
    }
    for (int a = 0; a < 3; a++) {
        b[a] = std::max(mn[a], ibox[a]);
        b[3 + a] = std::min(mx[a], ibox[3 + a]);
    }
}
}  // namespace

int buildInstancedTree(const InstancedIn& in, InstancedTree& out) {
    const int nm = in.nMeshes;
    const int64_t ni = in.nInst;
    std::vector<Wide8> blas((size_t)nm);
    std::vector<uint32_t>& shade = out.shade;   // 12 dwords per mesh primitive
    shade.clear();
    int64_t gTotal = 0;
    std::string err;
    // each mesh's primitive records, boxes and ranks; its tree is built once the instances' reach
    // into its object space is known (below)
    std::vector<std::vector<uint32_t>> meshPrims((size_t)nm), meshRank((size_t)nm);
    std::vector<std::vector<float>> meshBoxes((size_t)nm);
    for (int m = 0; m < nm; m++) {
        const int64_t n = in.meshCount[(size_t)m], first = in.meshFirst[(size_t)m];
        std::vector<uint32_t>&prims = meshPrims[(size_t)m], &rank = meshRank[(size_t)m];
        std::vector<float>& boxes = meshBoxes[(size_t)m];
        prims.assign((size_t)n * kW8PrimDwords, 0u);
        rank.resize((size_t)n);
        boxes.resize((size_t)n * 6);
        shade.resize((size_t)(gTotal + n) * 12, 0u);
        for (int64_t k = 0; k < n; k++) {
            const pt_object& o = in.objs[(size_t)(first + k)];
            primRecord(o, (uint32_t)k, &prims[(size_t)k * kW8PrimDwords], &boxes[(size_t)k * 6]);   // id: the object within its mesh
            meshShadeRecord(o, (uint32_t)k, in.mats, &shade[(size_t)(gTotal + k) * 12]);
            rank[(size_t)k] = (uint32_t)(gTotal + k);
        }
        gTotal += n;
    }
    int gBits = 1;
    while (((int64_t)1 << gBits) < gTotal) gBits++;
    if (gBits > 28 || ni > ((int64_t)1 << (30 - gBits)))
        return fail(PT_ERR_INVALID, "instanced scene: too many instances for the hit key (instance << " +
                                        std::to_string(gBits) + " | primitive)");
    // instances: world-to-object transforms, world boxes (every mesh vertex transformed, in double)
    InstRecords rec;
    int rc = instanceRecords(in, rec);
    if (rc) return rc;
    std::vector<std::array<double, 6>> ibox((size_t)ni);   // world box of each instance
    std::vector<uint32_t> used;
    double wmn[3] = {INFINITY, INFINITY, INFINITY}, wmx[3] = {-INFINITY, -INFINITY, -INFINITY};   // the world box
    for (int64_t i = 0; i < ni; i++) {
        const pt_instance& I = in.inst[(size_t)i];
        const int64_t first = in.meshFirst[(size_t)I.mesh], n = in.meshCount[(size_t)I.mesh];
        if (n == 0) continue;
        instanceWorldBox(I, in.objs + first, n, ibox[(size_t)i].data(), wmn, wmx);
        used.push_back((uint32_t)i);
    }
    if (used.empty()) return fail(PT_ERR_STATE, "instanced scene: no instance of a non-empty mesh");
    // The scene scalars and each mesh's reach.  A dynamic scene's mesh trees are quantised for twice
    // the reach, so that ordinary motion stays within it and the later builds keep the trees.
    std::vector<double>& reach = out.reach;
    InstScalars sc;
    instanceScalars(in, wmn, wmx, rec.w2o, sc, reach);
    if (in.dynamic)
        for (double& r : reach) r *= 2.0;
    int maxDepthB = 0;
    for (int m = 0; m < nm; m++) {
        const int64_t n = in.meshCount[(size_t)m];
        if (n > 0 && !buildWide8(meshPrims[(size_t)m].data(), meshBoxes[(size_t)m].data(), meshRank[(size_t)m].data(),
                                 n, blas[(size_t)m], err, reach[(size_t)m]))
            return fail(PT_ERR_STATE, err);
        maxDepthB = std::max(maxDepthB, blas[(size_t)m].depth);
    }
    // top-level leaves: per instance, its mesh root's internal children (re-braided; rebraid 0:
    // the mesh root), each with the world box of its object-space box (8 corners in double)
    std::vector<std::vector<SubRoot>> sub((size_t)nm);
    for (int m = 0; m < nm; m++) {
        const double inf[6] = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
        if (in.entryBudget > 0) meshSubRootsBudget(blas[(size_t)m], (size_t)in.entryBudget, sub[(size_t)m]);   // (A/B: surface-area-chosen partial re-braiding)
        else if (in.rebraid > 0) meshSubRoots(blas[(size_t)m], 0u, inf, in.rebraid, sub[(size_t)m]);
        if (sub[(size_t)m].size() == 1) sub[(size_t)m].clear();   // (the root itself)
    }
    std::vector<InstEntry>& entries = out.entries;
    entries.clear();
    std::vector<float> iboxes;
    auto addEntry = [&](uint32_t i, uint32_t mesh, uint32_t slot, const double* b) {
        for (int r = 0; r < 3; r++) iboxes.push_back(std::nextafter((float)b[r], -INFINITY));
        for (int r = 0; r < 3; r++) iboxes.push_back(std::nextafter((float)b[3 + r], INFINITY));
        entries.push_back({i, mesh, slot});
    };
    for (uint32_t i : used) {
        const pt_instance& I = in.inst[(size_t)i];
        const std::vector<SubRoot>& sr = sub[(size_t)I.mesh];
        if (sr.empty()) {
            addEntry(i, (uint32_t)I.mesh, 0u, ibox[(size_t)i].data());
            continue;
        }
        for (const SubRoot& r : sr) {
            double b[6];
            subRootWorldBox(I, r.box, ibox[(size_t)i].data(), b);
            addEntry(i, (uint32_t)I.mesh, r.slot, b);
        }
    }
    Wide8 top;
    if (!instanceTop(rec, entries, iboxes.data(), top, err)) return fail(PT_ERR_STATE, err);
    // layout: the top level from slot 0, then each mesh's tree (child and primitive bases relocated).
    // A dynamic scene reserves the top level's region at its upper bound for this number of entries
    // (its slot count changes with the matrices), so that later builds rewrite that region alone.
    uint32_t topSlots = (uint32_t)(top.nodes.size() / kW8NodeDwords);
    if (in.dynamic) {
        const int64_t cap = instanceTopSlots((int64_t)entries.size());
        if ((int64_t)topSlots > cap || cap >= ((int64_t)1 << 24))
            return fail(PT_ERR_STATE, "instanced BVH: top level beyond its reserved node slots");
        topSlots = (uint32_t)cap;
        top.nodes.resize((size_t)cap * kW8NodeDwords, 0u);
    }
    std::vector<uint32_t>& meshRoot = out.meshRoot;
    meshRoot.assign((size_t)nm, 0u);
    uint32_t nodeBase = topSlots, primBase = 0;
    for (int m = 0; m < nm; m++) {
        meshRoot[(size_t)m] = nodeBase;
        relocateWide8(blas[(size_t)m], nodeBase, primBase);
        nodeBase += (uint32_t)(blas[(size_t)m].nodes.size() / kW8NodeDwords);
        primBase += (uint32_t)(blas[(size_t)m].prims.size() / kW8PrimDwords);
    }
    if ((int64_t)nodeBase >= ((int64_t)1 << 24)) return fail(PT_ERR_STATE, "instanced BVH: more than 2^24 node slots");
    for (size_t k = 0; k < top.nodes.size(); k += kW8NodeDwords)
        if (top.nodes[k + 3] == kW8InstanceFlag) {
            top.nodes[k + 4] += meshRoot[top.nodes[k + 6]];
            top.nodes[k + 6] = 0u;
        }
    out.nodes = std::move(top.nodes);
    out.prims.clear();
    for (int m = 0; m < nm; m++) {
        out.nodes.insert(out.nodes.end(), blas[(size_t)m].nodes.begin(), blas[(size_t)m].nodes.end());
        out.prims.insert(out.prims.end(), blas[(size_t)m].prims.begin(), blas[(size_t)m].prims.end());
    }
    if (out.prims.empty()) out.prims.assign(kW8PrimDwords, 0u);
    if (shade.empty()) shade.assign(12, 0u);
    out.winst = std::move(rec.winst);
    out.gBits = gBits;
    out.depth = top.depth + 1 + maxDepthB + 1;   // stack: top levels, the marker, the mesh's levels
    out.maxDepthB = maxDepthB;
    for (int a = 0; a < 4; a++) out.sceneCE[a] = sc.ce[a];
    out.mixLim = sc.mixLim;
    out.topCap = topSlots;
    out.desc.clear();
    out.subBoxes.clear();
    out.entryPrims.clear();
    out.entryRank.clear();
    if (in.dynamic) {   // what the later builds need (rebuildInstancedTop)
        out.desc.resize((size_t)ni);
        std::vector<int32_t> subFirst((size_t)nm, -1);
        std::vector<double>& subBoxes = out.subBoxes;
        for (int m = 0; m < nm; m++) {
            if (sub[(size_t)m].empty()) continue;
            subFirst[(size_t)m] = (int32_t)(subBoxes.size() / 6);
            for (const SubRoot& r : sub[(size_t)m]) subBoxes.insert(subBoxes.end(), r.box, r.box + 6);
        }
        size_t e = 0;
        for (int64_t i = 0; i < ni; i++) {
            const int mesh = in.inst[(size_t)i].mesh;
            InstBoxDesc& D = out.desc[(size_t)i];
            D = InstBoxDesc{};
            D.objFirst = (int32_t)in.meshFirst[(size_t)mesh];
            D.objCount = (int32_t)in.meshCount[(size_t)mesh];
            D.entryFirst = (int32_t)e;
            D.subFirst = subFirst[(size_t)mesh];
            D.entryCount = D.objCount == 0 ? 0 : (D.subFirst < 0 ? 1 : (int32_t)sub[(size_t)mesh].size());
            e += (size_t)D.entryCount;
        }
        if (e != entries.size()) return fail(PT_ERR_STATE, "instanced BVH: entry count mismatch");
        if (subBoxes.empty()) subBoxes.assign(6, 0.0);
        const size_t ne = entries.size();
        out.entryPrims.assign(ne * kW8PrimDwords, 0u);
        out.entryRank.resize(ne);
        for (size_t k = 0; k < ne; k++) {
            out.entryPrims[k * kW8PrimDwords + 7] = (uint32_t)k;
            out.entryRank[k] = (uint32_t)k;
        }
    }
    if (wideStackFor(out.depth) < 0) return fail(PT_ERR_STATE, "instanced BVH too deep");
    return PT_OK;
}

}  // namespace pt
