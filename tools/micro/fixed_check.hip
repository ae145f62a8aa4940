// Sample mode's fixed-point conversions (csrc/pt_math.hpp) against plain references, on the GPU,
// with the kernels' own compiler flags.  Prints one JSON line; exit status 0 only when all match.
//
// blockFixed(x), float -> 32.32 fixed point, for all 2^32 fp32 bit patterns (negatives, +-0,
// denormals, sums >= 2^24, +-inf, NaN) against the oracle's rule evaluated beside it in fp64, where
// the product x * 2^32 is exact: NaN -> 0, clamp to +-2^62, truncate toward zero.
//
// fixedToFloat(a), the resolve pass's int64 -> float, against the same expression evaluated on the
// host, for the edge values {0, +-1, +-(2^32 - 1), +-2^32, +-(2^53 +- 1), +-2^62, INT64_MIN,
// INT64_MAX} and 2^24 values of every magnitude from a fixed 64-bit LCG.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "pt_math.hpp"

__global__ __launch_bounds__(256) void checkBlockFixed(uint64_t base, unsigned long long* out) {
    unsigned long long m = 0ull, n = 0ull;
    uint32_t firstBad = 0u;
    // each thread: 16 consecutive patterns
    const uint64_t first = base + ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
    for (int k = 0; k < 16; k++) {
        const uint32_t bits = (uint32_t)(first + (uint64_t)k);
        const float x = __uint_as_float(bits);
        double p = (double)x * 4294967296.0;
        if (p != p) p = 0.0;
        p = p < -0x1p62 ? -0x1p62 : (p > 0x1p62 ? 0x1p62 : p);
        const long long ref = (long long)p;
        const bool bad = blockFixed(x) != (unsigned long long)ref;
        if (bad && m == 0ull) firstBad = bits;
        m += bad ? 1ull : 0ull;
        n++;
    }
    // (patterns checked: one atomic per wave, not 2^28 on one address)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&out[0], n);
    if (m) {
        atomicAdd(&out[1], m);
        atomicMin(&out[2], (unsigned long long)firstBad);   // the lowest mismatching pattern
    }
}

__global__ __launch_bounds__(256) void runFixedToFloat(const unsigned long long* __restrict__ in, float* __restrict__ out,
                                                       size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = fixedToFloat(in[i]);
}

static float hostFixedToFloat(unsigned long long a) { return (float)((double)(long long)a * 0x1p-32); }

#define TRY(x)                                                                  \
    do {                                                                        \
        const hipError_t e_ = (x);                                              \
        if (e_ != hipSuccess) {                                                 \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));            \
            return 2;                                                           \
        }                                                                       \
    } while (0)

int main() {
    unsigned long long* dOut = nullptr;
    TRY(hipMalloc(&dOut, 3 * sizeof(unsigned long long)));
    const unsigned long long init[3] = {0ull, 0ull, ~0ull};
    TRY(hipMemcpy(dOut, init, sizeof(init), hipMemcpyHostToDevice));
    const uint64_t perLaunch = 1ull << 28;   // 2^28 patterns: 65,536 blocks of 256 threads x 16
    for (uint64_t base = 0; base < (1ull << 32); base += perLaunch)
        hipLaunchKernelGGL(checkBlockFixed, dim3((unsigned)(perLaunch / (256 * 16))), dim3(256), 0, 0, base, dOut);
    TRY(hipGetLastError());

    // fixedToFloat: the edges first, then the LCG's values (Knuth's MMIX multiplier and increment;
    // each value is one draw shifted right, arithmetically, by the top six bits of the next: every
    // magnitude and both signs)
    std::vector<unsigned long long> in;
    const long long p53 = 1ll << 53;
    const long long edges[] = {0ll, 1ll, -1ll, (1ll << 32) - 1, -((1ll << 32) - 1), 1ll << 32, -(1ll << 32),
                               p53 - 1, p53 + 1, -(p53 - 1), -(p53 + 1), 1ll << 62, -(1ll << 62), INT64_MIN, INT64_MAX};
    const size_t nEdges = sizeof(edges) / sizeof(edges[0]);
    for (size_t i = 0; i < nEdges; i++) in.push_back((unsigned long long)edges[i]);
    const size_t nRandom = (size_t)1 << 24;
    unsigned long long s = 0x243f6a8885a308d3ull;
    for (size_t i = 0; i < nRandom; i++) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const long long v = (long long)s;
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        in.push_back((unsigned long long)(v >> (int)(s >> 58)));
    }
    const size_t n = in.size();
    unsigned long long* dIn = nullptr;
    float* dF = nullptr;
    TRY(hipMalloc(&dIn, n * sizeof(unsigned long long)));
    TRY(hipMalloc(&dF, n * sizeof(float)));
    TRY(hipMemcpy(dIn, in.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(runFixedToFloat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dIn, dF, n);
    TRY(hipGetLastError());
    TRY(hipDeviceSynchronize());
    std::vector<float> got(n);
    TRY(hipMemcpy(got.data(), dF, n * sizeof(float), hipMemcpyDeviceToHost));
    unsigned long long hOut[3] = {0ull, 0ull, 0ull};
    TRY(hipMemcpy(hOut, dOut, sizeof(hOut), hipMemcpyDeviceToHost));

    unsigned long long edgeMis = 0ull, randomMis = 0ull;
    for (size_t i = 0; i < n; i++) {
        const float want = hostFixedToFloat(in[i]);
        if (std::memcmp(&want, &got[i], sizeof(float)) != 0) (i < nEdges ? edgeMis : randomMis)++;
    }
    printf("{\"block_fixed_checked\": %llu, \"block_fixed_mismatches\": %llu, \"block_fixed_first_mismatch\": %lld, "
           "\"fixed_to_float_edges\": %zu, \"fixed_to_float_edge_mismatches\": %llu, "
           "\"fixed_to_float_random\": %zu, \"fixed_to_float_random_mismatches\": %llu}\n",
           hOut[0], hOut[1], hOut[1] ? (long long)hOut[2] : -1ll, nEdges, edgeMis, nRandom, randomMis);
    (void)hipFree(dIn);
    (void)hipFree(dF);
    (void)hipFree(dOut);
    return (hOut[0] == (1ull << 32) && hOut[1] == 0ull && edgeMis == 0ull && randomMis == 0ull) ? 0 : 1;
}
