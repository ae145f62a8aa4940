/*
 * shim.h — the few CUDA names the reference's headers use, as plain host C++ (TEST INFRASTRUCTURE).
 *
 * Force-included (-include) in front of ref_driver.cpp, which then includes the build-time copies
 * of the reference's utils/ and simulation/ headers and the few functions cut out of its main.cu
 * (oracle/ref/build_ref.py).  Nothing here restates the reference: the shim only supplies what the
 * CUDA toolchain would, so that the reference's own text is what gets compiled and measured.
 *
 *   __host__ / __device__ / __global__   empty
 *   threadIdx, blockIdx, blockDim, gridDim   thread-local, set by whoever "launches"
 *   __syncthreads()                      a barrier over ALL lanes of a launch; a lane that returns
 *                                        drops out of it (the reading of generateLBVH this project
 *                                        follows)
 *   REF_LAUNCH / REF_LAUNCH_SYNC         what build_ref.py rewrites kernel<<<g, b>>>(...) into: a
 *                                        sequential loop over the grid, or one fibre per lane
 *                                        for a kernel whose body calls __syncthreads
 *   cuda* memory calls                   libc (cudaMalloc zero-fills)
 *   curandState                          the oracle's XORWOW (pt_oracle.cpp, pinned by
 *                                        tests/test_rocrand_pin.py), or a scripted tape of uniforms
 *   powf                                 switch ref_shim::g_powf_libm: 0 (default) evaluates
 *                                        powf(x, 5) as ((x*x)*(x*x))*x, the oracle's documented
 *                                        deviation; 1 leaves libm's powf
 */
#ifndef PT_REF_SHIM_H
#define PT_REF_SHIM_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include <ucontext.h>

#define __host__
#define __device__
#define __global__

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct int2 { int x, y; };
inline int2 make_int2(int x, int y) { return {x, y}; }

inline thread_local dim3 threadIdx(0, 0, 0), blockIdx(0, 0, 0), blockDim, gridDim;

inline int __clz(unsigned v) { return v ? __builtin_clz(v) : 32; }
inline int __clzll(unsigned long long v) { return v ? __builtin_clzll(v) : 64; }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }

/* ------------------------------------------------------------------ memory and error calls */
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
inline cudaError_t cudaMalloc(void** p, size_t n) { *p = calloc(n ? n : 1, 1); return *p ? cudaSuccess : 2; }
inline cudaError_t cudaMallocManaged(void** p, size_t n) { return cudaMalloc(p, n); }
inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) { memcpy(d, s, n); return cudaSuccess; }
inline cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t e) { return e == cudaSuccess ? "no error" : "host allocation failed"; }

/* ------------------------------------------------------------------------------ cuRAND */
extern "C" {
void orc_xorwow_init(uint64_t seed, uint64_t subsequence, uint32_t state[6]);
float orc_curand_uniform(uint32_t state[6]);
}
struct curandState {
    uint32_t s[6];        /* {d, v0..v4}: the oracle's and pt_film_get_rng's layout */
    const float* tape;    /* non-null: curand_uniform replays tape[0 .. tape_len), then 0.5f */
    int tape_len, used;   /* draws taken, in either mode */
};
inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long, curandState* st) {
    orc_xorwow_init(seed, subsequence, st->s);
    st->tape = nullptr;
    st->tape_len = st->used = 0;
}
inline float curand_uniform(curandState* st) {
    const int k = st->used++;
    if (st->tape) return k < st->tape_len ? st->tape[k] : 0.5f;
    return orc_curand_uniform(st->s);
}

/* ------------------------------------------------------------------- launches and barriers */
namespace ref_shim {

/* A launch whose kernel calls __syncthreads runs every lane as a fibre of one host thread: the
 * scheduler resumes each live lane in turn until it reaches the barrier or returns, and starts the
 * next phase once all of them have.  That is a barrier over the whole grid that a returned lane has
 * dropped out of, the same on every host (no thread limits, no scheduling noise), and 5,056 lanes
 * take milliseconds. */
struct Fiber {
    ucontext_t ctx;
    std::unique_ptr<char[]> stack;
    dim3 t, b;
    bool done = false;
};
inline ucontext_t g_scheduler;
inline Fiber* g_lane = nullptr;          /* the fibre running now, if any */
inline void (*g_call)(void*) = nullptr;  /* calls the launch's body */
inline void* g_body = nullptr;

inline void fiber_entry() {
    Fiber* self = g_lane;
    g_call(g_body);
    self->done = true;   /* returning resumes the scheduler (uc_link) */
}

template <class F> void run_grid(dim3 g, dim3 b, bool lanes_as_fibres, F body) {
    std::vector<std::unique_ptr<Fiber>> lanes;
    for (unsigned bz = 0; bz < g.z; bz++) for (unsigned by = 0; by < g.y; by++) for (unsigned bx = 0; bx < g.x; bx++)
    for (unsigned tz = 0; tz < b.z; tz++) for (unsigned ty = 0; ty < b.y; ty++) for (unsigned tx = 0; tx < b.x; tx++) {
        if (lanes_as_fibres) {
            lanes.emplace_back(new Fiber);
            lanes.back()->t = dim3(tx, ty, tz);
            lanes.back()->b = dim3(bx, by, bz);
            continue;
        }
        threadIdx = dim3(tx, ty, tz); blockIdx = dim3(bx, by, bz); blockDim = b; gridDim = g;
        body();
    }
    if (!lanes_as_fibres) return;
    const size_t kStack = 64 * 1024;
    g_body = &body;
    g_call = [](void* p) { (*static_cast<F*>(p))(); };
    for (auto& l : lanes) {
        l->stack.reset(new char[kStack]);
        getcontext(&l->ctx);
        l->ctx.uc_stack.ss_sp = l->stack.get();
        l->ctx.uc_stack.ss_size = kStack;
        l->ctx.uc_link = &g_scheduler;
        makecontext(&l->ctx, fiber_entry, 0);
    }
    for (size_t live = lanes.size(); live;) {   /* one pass = one phase between two barriers */
        for (auto& l : lanes) {
            if (l->done) continue;
            threadIdx = l->t; blockIdx = l->b; blockDim = b; gridDim = g;
            g_lane = l.get();
            swapcontext(&g_scheduler, &l->ctx);
            g_lane = nullptr;
            if (l->done) live--;
        }
    }
}

template <class K> auto launch(K kernel, dim3 g, dim3 b, bool lanes_as_fibres) {
    return [=](auto... args) { run_grid(g, b, lanes_as_fibres, [&] { kernel(args...); }); };
}

inline int g_powf_libm = 0;
inline float powf_switch(float x, float y) {
    if (!g_powf_libm && y == 5.0f) { const float x2 = x * x; return (x2 * x2) * x; }
    return ::powf(x, y);
}

}  // namespace ref_shim

inline void __syncthreads() {   /* back to the scheduler until every live lane has arrived */
    if (ref_shim::g_lane) swapcontext(&ref_shim::g_lane->ctx, &ref_shim::g_scheduler);
}

#define REF_LAUNCH(kernel, grid, block) ref_shim::launch(kernel, dim3(grid), dim3(block), false)
#define REF_LAUNCH_SYNC(kernel, grid, block) ref_shim::launch(kernel, dim3(grid), dim3(block), true)

#define powf(x, y) ref_shim::powf_switch((x), (y))

#endif
