// pt_temporal.hip — pt_film_temporal's pass: reproject the film's accumulated history into the new
// camera, test it against the first-hit guides and blend (the temporal half of SVGF-style denoisers).
// include/pt.h states the rule; every operation below is one rounded fp32 operation in its written
// order (-ffp-contract=off, IEEE division and square root, denormals kept), which tests/temporal_ref.py
// restates in numpy and the GPU tests hold bit for bit.
//
// One lane per pixel, 32 x 8 pixels per workgroup, no LDS.  A pixel reads its own record (three b128
// loads) and colour, gathers up to four history pixels around its reprojected position (three b128
// loads each; neighbouring lanes reproject to neighbouring history pixels wherever the surface is
// continuous, so the gathers of a wave fall on a few rows of the old image) and writes its colour, its
// length and the three rows of its new history pixel.  The measured time is in DESIGN.md section 10h.
#include "pt_temporal_dev.hpp"

namespace pt {
namespace {

constexpr int kTileW = 32, kTileH = 8;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kTileW * kTileH) void temporalKernel(const float* rgb, const float4* __restrict__ aov,
                                                                  const float4* __restrict__ prev, float4* __restrict__ next,
                                                                  float* out, float* __restrict__ outLen,
                                                                  const TemporalParams K) {
    const int W = K.width, H = K.height;
    const int x = (int)blockIdx.x * kTileW + (int)threadIdx.x, y = (int)blockIdx.y * kTileH + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 P0 = aov[3 * p], P1 = aov[3 * p + 1], P2 = aov[3 * p + 2];   // {albedo, depth}{n, obj}{p, mat}
    const float cr = rgb[3 * p], cg = rgb[3 * p + 1], cb = rgb[3 * p + 2];
    const float curR = K.linear ? cr : cr * cr, curG = K.linear ? cg : cg * cg, curB = K.linear ? cb : cb * cb;
    const bool hitP = __float_as_int(P1.w) >= 0;
    float ahR = 0.0f, ahG = 0.0f, ahB = 0.0f, al = 0.0f, ws = 0.0f;
    if (K.haveHistory && hitP) {
        const float ax = K.ll[0] - K.o[0], ay = K.ll[1] - K.o[1], az = K.ll[2] - K.o[2];
        const float wx = P2.x - K.o[0], wy = P2.y - K.o[1], wz = P2.z - K.o[2];
        const float hx = K.hor[0], hy = K.hor[1], hz = K.hor[2];
        const float vx = K.ver[0], vy = K.ver[1], vz = K.ver[2];
        const float cvwX = vy * wz - vz * wy, cvwY = vz * wx - vx * wz, cvwZ = vx * wy - vy * wx;   // cross(ver, w)
        const float cwhX = wy * hz - wz * hy, cwhY = wz * hx - wx * hz, cwhZ = wx * hy - wy * hx;   // cross(w, hor)
        const float chvX = hy * vz - hz * vy, chvY = hz * vx - hx * vz, chvZ = hx * vy - hy * vx;   // cross(hor, ver)
        const float den = dot3(hx, hy, hz, cvwX, cvwY, cvwZ);
        const float u = (-dot3(ax, ay, az, cvwX, cvwY, cvwZ)) / den;
        const float v = (-dot3(ax, ay, az, cwhX, cwhY, cwhZ)) / den;
        const float k = dot3(ax, ay, az, chvX, chvY, chvZ) / den;
        const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
        if (k > 0.0f && fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {   // (a NaN rejects)
            const float x0 = floorf(fx), y0 = floorf(fy);
            const float tx = fx - x0, ty = fy - y0;
            const int ix = (int)x0, iy = (int)y0;   // in [-1, W - 1], [-1, H - 1]
            const float planeLim = K.sigmaPlane * P0.w;
            const int matP = __float_as_int(P2.w);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int qy = iy + j;
                if (qy < 0 || qy >= H) continue;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int qx = ix + i;
                    if (qx < 0 || qx >= W) continue;
                    const float wq = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                    const float4 Q0 = prev[3 * q], Q1 = prev[3 * q + 1], Q2 = prev[3 * q + 2];   // {acc, len}{n, mat}{p, hit}
                    if (__float_as_int(Q2.w) == 0) continue;
                    if (__float_as_int(Q1.w) != matP) continue;
                    if (!(dot3(P1.x, P1.y, P1.z, Q1.x, Q1.y, Q1.z) >= K.normalCos)) continue;
                    if (!(fabsf(dot3(P1.x, P1.y, P1.z, Q2.x - P2.x, Q2.y - P2.y, Q2.z - P2.z)) <= planeLim)) continue;
                    if (!((fabsf(Q0.x) + fabsf(Q0.y)) + fabsf(Q0.z) < INFINITY)) continue;
                    if (!(wq > 0.0f)) continue;
                    ahR = ahR + wq * Q0.x;
                    ahG = ahG + wq * Q0.y;
                    ahB = ahB + wq * Q0.z;
                    al = al + wq * Q0.w;
                    ws = ws + wq;
                }
            }
        }
    }
    const bool have = ws > 0.0f;
    float len = 1.0f, accR = curR, accG = curG, accB = curB;
    if (have) {
        const float hR = ahR / ws, hG = ahG / ws, hB = ahB / ws, nh = al / ws;
        len = fminf(nh + 1.0f, K.maxHistory);
        const float alpha = 1.0f / len;
        accR = hR + (curR - hR) * alpha;
        accG = hG + (curG - hG) * alpha;
        accB = hB + (curB - hB) * alpha;
    }
    out[3 * p] = K.linear ? accR : sqrtf(accR);
    out[3 * p + 1] = K.linear ? accG : sqrtf(accG);
    out[3 * p + 2] = K.linear ? accB : sqrtf(accB);
    if (outLen) outLen[p] = len;
    next[3 * p] = make_float4(accR, accG, accB, len);
    next[3 * p + 1] = make_float4(P1.x, P1.y, P1.z, P2.w);
    next[3 * p + 2] = make_float4(P2.x, P2.y, P2.z, __int_as_float(hitP ? 1 : 0));
}

}  // namespace

hipError_t temporalPass(const float* rgb, const pt_aov* aov, const void* prev, void* next, float* out, float* outLen,
                        const TemporalParams& params, hipStream_t stream) {
    if (params.width <= 0 || params.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((params.width + kTileW - 1) / kTileW), (unsigned)((params.height + kTileH - 1) / kTileH));
    temporalKernel<<<grid, dim3(kTileW, kTileH), 0, stream>>>(rgb, reinterpret_cast<const float4*>(aov),
                                                              static_cast<const float4*>(prev), static_cast<float4*>(next),
                                                              out, outLen, params);
    return hipGetLastError();
}

}  // namespace pt
