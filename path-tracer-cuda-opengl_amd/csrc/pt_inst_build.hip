// pt_inst_build.hip — world boxes of the instances and of their top-level entries, the top level's
// instance records and the world-space light records of PT_BVH_LIGHTS (pt_inst_dev.hpp).
//
// One workgroup per instance.  Its lanes take the mesh's objects in turn, transform every vertex
// (a sphere: the eight corners of its box) by the instance's matrix in fp64 and keep the
// componentwise min / max; the partial boxes are reduced by wave shuffles, then across the
// workgroup's waves through LDS.  min and max are exact and order-free, and each transformed
// coordinate is the host's expression a0 * x + a1 * y + a2 * z + t evaluated left to right without
// contraction, so the box is the one buildInstancedTree computes.  The same workgroup then writes the
// instance's top-level entries: each sub-root's object-space box taken through the matrix (eight
// corners), clipped to the instance's exact box and rounded to float outward.
// One workgroup per instance whatever its mesh's size: the scenes this serves have many instances
// of meshes of thousands of objects (C5: 211 workgroups, 60 vertices per lane).  A single instance
// of a million-object mesh would run its 4,000 iterations per lane on one compute unit -- correct,
// a few milliseconds; splitting such a mesh over several workgroups with a second reduction pass is
// not done.
#include "pt_inst_dev.hpp"

#include "pt_wide8.hpp"

#include <cmath>

namespace pt {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// std::min / std::max as the host writes them (the first argument is kept when either is a NaN)
__device__ inline double minD(double a, double b) { return b < a ? b : a; }
__device__ inline double maxD(double a, double b) { return a < b ? b : a; }

// std::nextafter(x, -inf) and (x, +inf) for a float
__device__ inline float floatBelow(float x) {
    if (x != x || x == -INFINITY) return x;
    if (x == 0.0f) return __uint_as_float(0x80000001u);
    const uint32_t u = __float_as_uint(x);
    return __uint_as_float(x > 0.0f ? u - 1u : u + 1u);
}
__device__ inline float floatAbove(float x) {
    if (x != x || x == INFINITY) return x;
    if (x == 0.0f) return __uint_as_float(0x00000001u);
    const uint32_t u = __float_as_uint(x);
    return __uint_as_float(x > 0.0f ? u + 1u : u - 1u);
}

__global__ __launch_bounds__(kBlock) void instBoxKernel(const pt_object* __restrict__ objs, const float* __restrict__ mats,
                                                        const InstBoxDesc* __restrict__ desc,
                                                        const double* __restrict__ sub, double* __restrict__ ibox,
                                                        float* __restrict__ ebox) {
    __shared__ double part[kWaves][6];
    __shared__ double box[6];
    const int64_t i = blockIdx.x;
    const InstBoxDesc D = desc[i];
    const float* M = mats + 12 * i;
    double a[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) a[r][c] = (double)M[4 * r + c];
        t[r] = (double)M[4 * r + 3];
    }
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto grow = [&](double x, double y, double z) {
        for (int r = 0; r < 3; r++) {
            const double w = a[r][0] * x + a[r][1] * y + a[r][2] * z + t[r];
            mn[r] = minD(mn[r], w);
            mx[r] = maxD(mx[r], w);
        }
    };
    for (int k = (int)threadIdx.x; k < D.objCount; k += kBlock) {
        const pt_object o = objs[(int64_t)D.objFirst + k];
        if (o.type == PT_SPHERE) {
            const double rr = fabs((double)o.v[3]);
            for (int c = 0; c < 8; c++)
                grow(o.v[0] + ((c & 1) ? rr : -rr), o.v[1] + ((c & 2) ? rr : -rr), o.v[2] + ((c & 4) ? rr : -rr));
        } else {
            for (int v = 0; v < 3; v++) grow(o.v[3 * v], o.v[3 * v + 1], o.v[3 * v + 2]);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int r = 0; r < 3; r++) {
            mn[r] = minD(mn[r], __shfl_xor(mn[r], off, 64));
            mx[r] = maxD(mx[r], __shfl_xor(mx[r], off, 64));
        }
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0)
        for (int r = 0; r < 3; r++) { part[wave][r] = mn[r]; part[wave][3 + r] = mx[r]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int r = (int)threadIdx.x;
        double v = part[0][r];
        for (int w = 1; w < kWaves; w++) v = r < 3 ? minD(v, part[w][r]) : maxD(v, part[w][r]);
        box[r] = v;
        ibox[6 * i + r] = v;
    }
    __syncthreads();
    for (int e = (int)threadIdx.x; e < D.entryCount; e += kBlock) {
        double b[6];
        if (D.subFirst < 0) {
            for (int r = 0; r < 6; r++) b[r] = box[r];
        } else {
            const double* S = sub + 6 * ((int64_t)D.subFirst + e);
            double en[3] = {INFINITY, INFINITY, INFINITY}, ex[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int c = 0; c < 8; c++) {
                const double q[3] = {S[(c & 1) ? 3 : 0], S[(c & 2) ? 4 : 1], S[(c & 4) ? 5 : 2]};
                for (int r = 0; r < 3; r++) {
                    const double w = a[r][0] * q[0] + a[r][1] * q[1] + a[r][2] * q[2] + t[r];
                    en[r] = minD(en[r], w);
                    ex[r] = maxD(ex[r], w);
                }
            }
            for (int r = 0; r < 3; r++) {   // (never beyond the instance's exact box)
                b[r] = maxD(en[r], box[r]);
                b[3 + r] = minD(ex[r], box[3 + r]);
            }
        }
        float* out = ebox + 6 * ((int64_t)D.entryFirst + e);
        for (int r = 0; r < 3; r++) {
            out[r] = floatBelow((float)b[r]);
            out[3 + r] = floatAbove((float)b[3 + r]);
        }
    }
}

// The top level's leaf children -> instance records (what pt::instanceLeaves does on the host).  One
// thread per node slot of the top level, which was zeroed before the build: a slot that holds a node
// has children (meta bytes); an unused slot and an instance record have none (dwords 6, 7 are 0 in
// both), so a thread that looks at a slot another thread is writing a record into leaves it alone
// whatever it sees.  A leaf child in slot j (meta (1 << 5) | offset: exactly one entry) becomes an
// internal child whose slot childBase + j holds the entry's record; the builder gave every node a
// child block, and checked childBase + 8 <= its slot cap.
__global__ void instRecordKernel(uint32_t* __restrict__ nodes, uint32_t slots, const uint32_t* __restrict__ wprims,
                                 const uint32_t* __restrict__ entries, uint32_t nEntries, const float* __restrict__ winst,
                                 const uint32_t* __restrict__ meshRoot, uint32_t* __restrict__ err) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    uint32_t* R = nodes + (size_t)kW8NodeDwords * s;
    if (R[3] == kW8InstanceFlag) return;
    uint32_t meta[2] = {R[6], R[7]};
    if ((meta[0] | meta[1]) == 0u) return;
    const uint32_t childBase = R[4], primBase = R[5];
    for (int j = 0; j < 8; j++) {
        const uint32_t mb = (meta[j >> 2] >> (8 * (j & 3))) & 0xffu;
        if (mb == 0u || (mb & 0x1fu) >= 24u) continue;
        const uint32_t prim = primBase + (mb & 0x1fu);
        if ((mb >> 5) != 1u || prim >= nEntries) {   // more than one entry in a leaf / a corrupt node
            atomicOr(err, 1u);
            continue;
        }
        const uint32_t e = wprims[(size_t)kW8PrimDwords * prim + 7];
        if (e >= nEntries) {
            atomicOr(err, 2u);
            continue;
        }
        const uint32_t inst = entries[3 * (size_t)e], mesh = entries[3 * (size_t)e + 1], slot = entries[3 * (size_t)e + 2];
        const float* W = winst + 16 * (size_t)inst;
        const uint32_t cls = __float_as_uint(W[13]);
        uint32_t* dst = nodes + (size_t)kW8NodeDwords * (childBase + (uint32_t)j);
        dst[0] = cls == 1u ? 1u : 0u;
        dst[1] = cls == 2u ? 1u : 0u;   // translation only: the kernels move the origin, keep the direction
        dst[2] = 0u;
        dst[3] = kW8InstanceFlag;
        dst[4] = meshRoot[mesh] + slot;
        dst[5] = inst;
        dst[6] = 0u;
        dst[7] = 0u;
        for (int k = 0; k < 12; k++) dst[8 + k] = __float_as_uint(W[k]);
        for (int k = 20; k < kW8NodeDwords; k++) dst[k] = 0u;
        meta[j >> 2] = (meta[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((0x20u | 24u | (uint32_t)j) << (8 * (j & 3)));
    }
    R[6] = meta[0];
    R[7] = meta[1];
}

// The sampled lights of an instanced scene (PT_BVH_LIGHTS; pt.h states the rule): one thread per record,
// = per (instance, emissive triangle of its mesh), records in flattened object order.  The record's
// instance is the last one whose first record is not beyond it (a binary search over n + 1 prefix
// sums: instances without lights share their successor's entry and are never the last); the triangle
// is the record's offset into its mesh's run of emissive objects.  Each vertex goes through the matrix
// in fp64, ((m0 * x + m1 * y) + m2 * z) + m3, one rounded operation each (-ffp-contract=off), and is
// rounded to fp32 once; the edges are fp32 differences of the rounded vertices, as the flat list's.
// A thread per record whatever the instance count: two records are one wave of one block, the
// 1.04 M records of every triangle of C5 emissive are 4,075 blocks.
__global__ __launch_bounds__(kBlock) void instLightKernel(const pt_object* __restrict__ objs, const float* __restrict__ mats,
                                                          const float* __restrict__ m, const uint32_t* __restrict__ first,
                                                          const uint32_t* __restrict__ src, const uint32_t* __restrict__ lobj,
                                                          uint32_t nInst, uint32_t nLights, float4* __restrict__ lights) {
    const uint32_t r = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (r >= nLights) return;
    uint32_t lo = 0u, hi = nInst;   // first[lo] <= r < first[hi] (first[0] = 0, first[nInst] = nLights)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= r) lo = mid;
        else hi = mid;
    }
    const pt_object o = objs[lobj[src[lo] + (r - first[lo])]];
    const float* M = m + 12 * (size_t)lo;
    float w[3][3];
    for (int v = 0; v < 3; v++) {
        const double x = (double)o.v[3 * v], y = (double)o.v[3 * v + 1], z = (double)o.v[3 * v + 2];
        for (int a = 0; a < 3; a++)
            w[v][a] = (float)((((double)M[4 * a] * x + (double)M[4 * a + 1] * y) + (double)M[4 * a + 2] * z) + (double)M[4 * a + 3]);
    }
    const float* E = mats + 8 * (size_t)o.mat;
    float4* L = lights + 4 * (size_t)r;
    L[0] = make_float4(w[0][0], w[0][1], w[0][2], 0.0f);
    L[1] = make_float4(w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2], 0.0f);
    L[2] = make_float4(w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2], 0.0f);
    L[3] = make_float4(E[0], E[1], E[2], 0.0f);
}

}  // namespace

hipError_t instanceLights(const InstLightIn& in, float4* lights, hipStream_t stream) {
    if (in.nLights == 0u) return hipSuccess;
    if (in.nInst == 0u) return hipErrorInvalidValue;
    instLightKernel<<<dim3((in.nLights + (uint32_t)kBlock - 1u) / (uint32_t)kBlock), dim3(kBlock), 0, stream>>>(
        in.objs, in.mats, in.m, in.first, in.src, in.obj, in.nInst, in.nLights, lights);
    return hipGetLastError();
}

hipError_t instanceRecords(uint32_t* nodes, uint32_t slots, const uint32_t* wprims, const uint32_t* entries, uint32_t nEntries,
                           const float* winst, const uint32_t* meshRoot, uint32_t* err, hipStream_t stream) {
    if (slots == 0u) return hipSuccess;
    instRecordKernel<<<dim3((slots + 255u) / 256u), dim3(256), 0, stream>>>(nodes, slots, wprims, entries, nEntries, winst,
                                                                            meshRoot, err);
    return hipGetLastError();
}

hipError_t instanceBoxes(const InstBoxIn& in, double* ibox, float* ebox, hipStream_t stream) {
    if (in.n <= 0) return hipSuccess;
    if (in.n > 0x7fffffff) return hipErrorInvalidValue;
    instBoxKernel<<<dim3((unsigned)in.n), dim3(kBlock), 0, stream>>>(in.objs, in.m, in.desc, in.sub, ibox, ebox);
    return hipGetLastError();
}

}  // namespace pt
