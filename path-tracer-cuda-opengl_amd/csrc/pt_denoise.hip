// pt_denoise.hip — one pass of pt_film_denoise: the edge-avoiding a-trous wavelet filter (Dammertz et
// al. 2010) guided by first-hit AOVs.  include/pt.h states the rule; every operation below is one
// rounded fp32 operation in its written order (-ffp-contract=off, IEEE division, denormals kept), which
// tests/atrous_ref.py restates in numpy and the GPU tests hold bit for bit.
//
// One lane per pixel, 32 x 8 pixels per workgroup (a row of a wave's lanes reads consecutive pixels: the
// three 16-byte rows of a tap's record are three b128 loads, its colour three dwords).  The 25 taps of
// a workgroup overlap at tap spacings 1 and 2 and are spread from 4 on; either way the guides and the
// image of a frame (1920 x 1080: 100 MB + 25 MB) are re-read through L2 / the Infinity Cache, not
// staged: the passes' measured times are in DESIGN.md section 10g.
#include "pt_denoise_dev.hpp"

namespace pt {
namespace {

constexpr int kTileW = 32, kTileH = 8;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kTileW * kTileH) void atrousKernel(const float* __restrict__ in, const float4* __restrict__ aov,
                                                                float* __restrict__ out, int W, int H, int step, float isa2,
                                                                float isc2, float sigmaPlane) {
    const int x = (int)blockIdx.x * kTileW + (int)threadIdx.x, y = (int)blockIdx.y * kTileH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 P0 = aov[3 * p], P1 = aov[3 * p + 1], P2 = aov[3 * p + 2];   // {albedo, depth}{n, obj}{p, mat}
    const bool hitP = __float_as_int(P1.w) >= 0;
    const float cx = in[3 * p], cy = in[3 * p + 1], cz = in[3 * p + 2];
    const float planeDen = sigmaPlane * P0.w;
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= W) continue;
            const float h = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
            float w, qr, qg, qb;
            if (dx == 0 && dy == 0) {
                w = h; qr = cx; qg = cy; qb = cz;
            } else {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                const float4 Q1 = aov[3 * q + 1];
                if ((__float_as_int(Q1.w) >= 0) != hitP) continue;
                const float4 Q0 = aov[3 * q];
                float wn = 1.0f, wp = 1.0f;
                if (hitP) {
                    const float4 Q2 = aov[3 * q + 2];
                    wn = fmaxf(0.0f, dot3(P1.x, P1.y, P1.z, Q1.x, Q1.y, Q1.z));
#pragma unroll
                    for (int r = 0; r < 6; r++) wn = wn * wn;
                    const float dist = fabsf(dot3(P1.x, P1.y, P1.z, Q2.x - P2.x, Q2.y - P2.y, Q2.z - P2.z));
                    const float xx = dist / planeDen;
                    wp = 1.0f / (1.0f + xx * xx);
                }
                const float dar = Q0.x - P0.x, dag = Q0.y - P0.y, dab = Q0.z - P0.z;
                const float wa = 1.0f / (1.0f + dot3(dar, dag, dab, dar, dag, dab) * isa2);
                qr = in[3 * q]; qg = in[3 * q + 1]; qb = in[3 * q + 2];
                const float dcr = qr - cx, dcg = qg - cy, dcb = qb - cz;
                const float wc = 1.0f / (1.0f + dot3(dcr, dcg, dcb, dcr, dcg, dcb) * isc2);
                w = (((h * wn) * wp) * wa) * wc;
            }
            if (!(w > 0.0f)) continue;   // 0 and NaN alike: not added (0 x inf never appears)
            ax = ax + w * qr;
            ay = ay + w * qg;
            az = az + w * qb;
            ws = ws + w;
        }
    }
    out[3 * p] = ax / ws;
    out[3 * p + 1] = ay / ws;
    out[3 * p + 2] = az / ws;
}

}  // namespace

hipError_t atrousPass(const float* in, const pt_aov* aov, float* out, int width, int height, int step, float isa2,
                      float isc2, float sigmaPlane, hipStream_t stream) {
    if (width <= 0 || height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH));
    atrousKernel<<<grid, dim3(kTileW, kTileH), 0, stream>>>(in, reinterpret_cast<const float4*>(aov), out, width, height,
                                                            step, isa2, isc2, sigmaPlane);
    return hipGetLastError();
}

}  // namespace pt
