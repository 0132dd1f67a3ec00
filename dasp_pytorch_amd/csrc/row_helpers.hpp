// What the row-walking effects share (fbdelay, fdn, phaser, tvfilter, moddelay; limiter, oversample and resample take the host helper):
// one workgroup owns a (b, c) row and walks it in steps or tiles whose waves talk through LDS. Every helper here was lifted out of
// those files under one rule: the device code of each file, compiled to assembly with the build's flags, is the same listing as before
// (profiles/r25/row_helpers). What could not be shared that way stayed where it was.
#pragma once

#include "common.hpp"

namespace dasp {

// The barrier of the steps: what the waves exchange goes through LDS only, so a wave waits for its own LDS operations and no more.
// __syncthreads() is also a fence for global memory: it would wait for the acknowledgement of every store of y, v or gx issued so far and
// for the loads of the next step's inputs - a memory round trip on the critical path of every step.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ring word of a position t in (-R, 2 R); the range holds by construction and is enforced all the same
__device__ __forceinline__ int ring_wrap(int t, int R) {
    t += t < 0 ? R : 0;
    t -= t >= R ? R : 0;
    return min(max(t, 0), R - 1);
}

// a = exp(-2 pi max(damping_hz, 0) / sr), the pole of the one-pole low-pass in a feedback path
__device__ __forceinline__ double damping_pole(double damping_hz, double sr) {
    const double dh = damping_hz < 0.0 ? 0.0 : damping_hz;                 // a NaN stays
    return exp(-6.283185307179586 * dh / sr);
}

// Catmull-Rom weights of four consecutive samples for a read at fraction f past the second of them, and their derivatives by f
struct CrW { float a, b, c, d; };
__device__ __forceinline__ CrW cr_weights(float f) {
    const float f2 = f * f;
    return CrW{0.5f * f * ((2.f - f) * f - 1.f), 0.5f * ((3.f * f - 5.f) * f2 + 2.f), 0.5f * f * ((4.f - 3.f * f) * f + 1.f), 0.5f * f2 * (f - 1.f)};
}
__device__ __forceinline__ CrW cr_dweights(float f) {
    return CrW{0.5f * ((4.f - 3.f * f) * f - 1.f), 0.5f * f * (9.f * f - 10.f), 0.5f * ((8.f - 9.f * f) * f + 1.f), 0.5f * f * (3.f * f - 2.f)};
}
// all four products, always: a NaN or inf sample under a zero weight is a NaN
__device__ __forceinline__ float cr_dot(const CrW& w, float t0, float t1, float t2, float t3) { return w.a * t0 + w.b * t1 + w.c * t2 + w.d * t3; }
__device__ __forceinline__ float cr_dot(const CrW& w, const float* xs) { return w.a * xs[0] + w.b * xs[1] + w.c * xs[2] + w.d * xs[3]; }

// v of the lane DPP names, or 1 where there is none (lanes shifted in from outside a row, rows the mask leaves out)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_or_one(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0x3f800000, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}

// consecutive samples per thread in a step of S: odd, so that the lanes' LDS words (stride spt) fall on distinct banks
template <int THREADS> __host__ __device__ __forceinline__ int odd_spt(int S) { return ((S + THREADS - 1) / THREADS) | 1; }

// A staged tile of THREADS x SPT samples: sample i at word i + i / SPT, so that threads reading SPT consecutive samples fall on distinct banks.
template <int SPT> __device__ __forceinline__ int stage_word(int i) { return i + i / SPT; }

// A tile from global memory, a lane per consecutive sample, one tile ahead of its use; what lies past the row is zero.
template <int SPT, int THREADS>
__device__ __forceinline__ void stage_load(float (&o)[SPT], const float* __restrict__ p, long t0, long N, int tid) {
    const bool live = t0 >= 0 && t0 < N;
#pragma unroll
    for (int m = 0; m < SPT; ++m) {
        const long n = t0 + tid + THREADS * m;
        const float v = p[live ? min(n, N - 1) : 0];
        o[m] = live && n < N ? v : 0.f;
    }
}
template <int SPT, int THREADS>
__device__ __forceinline__ void stage_put(float* st, const float (&v)[SPT], int tid) {
#pragma unroll
    for (int m = 0; m < SPT; ++m) st[stage_word<SPT>(tid + THREADS * m)] = v[m];
}

// what a C entry point returns after its launches
inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DASP_OK : (int)e;
}

}  // namespace dasp
