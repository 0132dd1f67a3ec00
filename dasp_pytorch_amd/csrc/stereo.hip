// Stereo utilities: stereo_widener, stereo_panner, stereo_bus - forward and backward, fused elementwise kernels with in-kernel
// control-gradient reduction. Replaces dasp_pytorch/functional.py:580-605 (widener), :608-636 (panner), :32-62 (bus) and their
// autograd graphs. All HBM-bound streaming kernels: one pass over the inputs, one over the outputs, nothing else moves.
//
// A workgroup handles one segment of ST_SEG samples of one "line" (a batch item for the widener, a (batch, track) row for the
// panner, a (batch, channel) row for the bus); backward kernels write one partial sum per (line, segment[, track]) and a finalize
// kernel reduces them in fp64 and applies the chain rule of the control.
#include "common.hpp"

namespace dasp {

constexpr int ST_THREADS = 256;
constexpr int ST_SEG = 4096;     // samples per workgroup: 4 float4 per thread

// STREAM: non-temporal hint, used by the backward kernels (several read streams + a write stream; elementwise.hip: 0.160 -> 0.132 ms)
template <bool STREAM = false> __device__ __forceinline__ f4 ld4(const float* p, long i, long n, bool vec) {
    if (vec) return STREAM ? ld_stream(reinterpret_cast<const f4*>(p + i)) : *reinterpret_cast<const f4*>(p + i);
    return f4{i < n ? p[i] : 0.f, i + 1 < n ? p[i + 1] : 0.f, i + 2 < n ? p[i + 2] : 0.f, i + 3 < n ? p[i + 3] : 0.f};
}
template <bool STREAM = false> __device__ __forceinline__ void st4(float* p, long i, long n, bool vec, f4 v) {
    if (vec) { if (STREAM) st_stream(reinterpret_cast<f4*>(p + i), v); else *reinterpret_cast<f4*>(p + i) = v; return; }
    if (i < n) p[i] = v.x;
    if (i + 1 < n) p[i + 1] = v.y;
    if (i + 2 < n) p[i + 2] = v.z;
    if (i + 3 < n) p[i + 3] = v.w;
}
__device__ __forceinline__ float dot4(f4 a, f4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// workgroup sum of `v`, written by thread 0 to *out
__device__ __forceinline__ void block_sum_to(float v, float* out) {
    __shared__ float red[ST_THREADS / 64];
    const float w = wave_sum(v);
    __syncthreads();                     // red may still be read from a previous call
    if (lane_id() == 0) red[wave_id()] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < ST_THREADS / 64; ++i) s += red[i];
        *out = s;
    }
}

// ---- widener: left = L + k R, right = k L + R, k = 1 - 2 width  (mid/side scaling of functional.py:592-603 multiplied out) -------
// x, y (B, 2, N); width (B). Backward (x = gy here, out = gx): the same map (it is symmetric); d/dwidth = -2 sum (R gL + L gR).
template <bool BWD>
__global__ void __launch_bounds__(ST_THREADS)
widener_kernel(const float* __restrict__ x, const float* __restrict__ width, const float* __restrict__ gy, float* __restrict__ out,
               float* __restrict__ partials, long N, int nseg, int vec) {
    const int b = blockIdx.x / nseg, seg = blockIdx.x % nseg;
    const float k = 1.f - 2.f * width[b];
    const float* xl = x + (size_t)b * 2 * N;
    const float* xr = xl + N;
    const float* src_l = BWD ? gy + (size_t)b * 2 * N : xl;
    const float* src_r = src_l + N;
    float* ol = out + (size_t)b * 2 * N;
    float* orr = ol + N;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < ST_SEG / (4 * ST_THREADS); ++j) {
        const long i = (long)seg * ST_SEG + (long)(j * ST_THREADS + threadIdx.x) * 4;
        if (i >= N) break;
        const f4 l = ld4<BWD>(src_l, i, N, vec), r = ld4<BWD>(src_r, i, N, vec);
        st4<BWD>(ol, i, N, vec, l + k * r);
        st4<BWD>(orr, i, N, vec, k * l + r);
        if (BWD) acc += dot4(ld4<true>(xr, i, N, vec), l) + dot4(ld4<true>(xl, i, N, vec), r);     // R gL + L gR
    }
    if (BWD) block_sum_to(-2.f * acc, partials + (size_t)b * nseg + seg);
}

// ---- panner: y[b, 0, t, :] = lg x[b, t, :], y[b, 1, t, :] = rg x[b, t, :]  (functional.py:621-634) -------------------------------
// theta = pan pi / 2, lg = sqrt((pi/2 - theta) (2/pi) cos theta), rg = sqrt(theta (2/pi) sin theta). x (B, T, N), pan (B * T), y (B, 2, T, N).
__device__ __forceinline__ void pan_gains(float pan, float& lg, float& rg) {
    const float hp = 1.57079632679489661923f, theta = pan * hp;
    lg = sqrtf((hp - theta) * (2.f / 3.14159265358979323846f) * cosf(theta));
    rg = sqrtf(theta * (2.f / 3.14159265358979323846f) * sinf(theta));
}
template <bool BWD>
__global__ void __launch_bounds__(ST_THREADS)
panner_kernel(const float* __restrict__ x, const float* __restrict__ pan, const float* __restrict__ gy, float* __restrict__ out,
              float* __restrict__ partials, int T, long N, int nseg, int vec) {
    const int row = blockIdx.x / nseg, seg = blockIdx.x % nseg;      // row = b * T + t
    const int b = row / T, t = row % T;
    float lg, rg;
    pan_gains(pan[row], lg, rg);
    const float* xr = x + (size_t)row * N;
    const size_t y0 = ((size_t)(b * 2) * T + t) * N, y1 = ((size_t)(b * 2 + 1) * T + t) * N;
    float al = 0.f, ar = 0.f;
#pragma unroll
    for (int j = 0; j < ST_SEG / (4 * ST_THREADS); ++j) {
        const long i = (long)seg * ST_SEG + (long)(j * ST_THREADS + threadIdx.x) * 4;
        if (i >= N) break;
        const f4 xv = ld4(xr, i, N, vec);
        if (!BWD) {
            st4(out + y0, i, N, vec, lg * xv);
            st4(out + y1, i, N, vec, rg * xv);
        } else {
            const f4 g0 = ld4<true>(gy + y0, i, N, vec), g1 = ld4<true>(gy + y1, i, N, vec);
            st4<true>(out + (size_t)row * N, i, N, vec, lg * g0 + rg * g1);
            al += dot4(xv, g0); ar += dot4(xv, g1);
        }
    }
    if (BWD) {
        block_sum_to(al, partials + ((size_t)row * nseg + seg) * 2);
        block_sum_to(ar, partials + ((size_t)row * nseg + seg) * 2 + 1);
    }
}

// ---- bus: y[b, c, :] = sum_t 10^(send_db[b, t] / 20) x[b, c, t, :]  (functional.py:49-59) ------------------------------------------
// x (B, 2, T, N), send_db (B * T), y (B, 2, N). Backward: gx[b, c, t, :] = s[b, t] gy[b, c, :]; partial[(b, c), seg, t] = sum gy x.
constexpr int ST_TMAX = 64;
template <bool BWD>
__global__ void __launch_bounds__(ST_THREADS)
bus_kernel(const float* __restrict__ x, const float* __restrict__ send_db, const float* __restrict__ gy, float* __restrict__ out,
           float* __restrict__ partials, int T, long N, int nseg, int vec) {
    __shared__ float s_lin[ST_TMAX];
    const int row = blockIdx.x / nseg, seg = blockIdx.x % nseg;      // row = b * 2 + c
    const int b = row >> 1;
    for (int t = threadIdx.x; t < T; t += ST_THREADS) s_lin[t] = exp10f(send_db[(size_t)b * T + t] * 0.05f);
    __syncthreads();
    const float* xr = x + (size_t)row * T * N;
    if (!BWD) {
#pragma unroll
        for (int j = 0; j < ST_SEG / (4 * ST_THREADS); ++j) {
            const long i = (long)seg * ST_SEG + (long)(j * ST_THREADS + threadIdx.x) * 4;
            if (i >= N) break;
            f4 acc = f4{0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < T; ++t) acc += s_lin[t] * ld4(xr + (size_t)t * N, i, N, vec);
            st4(out + (size_t)row * N, i, N, vec, acc);
        }
    } else {
        f4 g[ST_SEG / (4 * ST_THREADS)];
#pragma unroll
        for (int j = 0; j < ST_SEG / (4 * ST_THREADS); ++j) {
            const long i = (long)seg * ST_SEG + (long)(j * ST_THREADS + threadIdx.x) * 4;
            g[j] = i < N ? ld4(gy + (size_t)row * N, i, N, vec) : f4{0.f, 0.f, 0.f, 0.f};
        }
        for (int t = 0; t < T; ++t) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < ST_SEG / (4 * ST_THREADS); ++j) {
                const long i = (long)seg * ST_SEG + (long)(j * ST_THREADS + threadIdx.x) * 4;
                if (i >= N) break;
                acc += dot4(ld4<true>(xr + (size_t)t * N, i, N, vec), g[j]);
                st4<true>(out + ((size_t)row * T + t) * N, i, N, vec, s_lin[t] * g[j]);
            }
            block_sum_to(acc, partials + ((size_t)row * nseg + seg) * T + t);
        }
    }
}

// mode 0 widener: gctl[b] = sum_seg partials[b][seg]
// mode 1 panner:  gctl[row] = d lg/d pan * sum partial_l + d rg/d pan * sum partial_r   (fp64; zero where the gain is zero: pan = 0 or 1)
// mode 2 bus:     gctl[b * T + t] = ln10/20 s[b,t] * sum_{c, seg} partials[(b, c), seg, t]
__global__ void stereo_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ ctl, float* __restrict__ gctl, int n,
                                       int nseg, int T, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) {
        double s = 0.0;
        for (int k = 0; k < nseg; ++k) s += (double)partials[(size_t)i * nseg + k];
        gctl[i] = (float)s;
    } else if (mode == 1) {
        double sl = 0.0, sr = 0.0;
        for (int k = 0; k < nseg; ++k) { sl += (double)partials[((size_t)i * nseg + k) * 2]; sr += (double)partials[((size_t)i * nseg + k) * 2 + 1]; }
        const double hp = 1.57079632679489661923, th = (double)ctl[i] * hp, c = cos(th), sn = sin(th);
        const double ul = (hp - th) * (2.0 / 3.14159265358979323846) * c, ur = th * (2.0 / 3.14159265358979323846) * sn;   // lg^2, rg^2
        const double dul = (2.0 / 3.14159265358979323846) * (-c - (hp - th) * sn), dur = (2.0 / 3.14159265358979323846) * (sn + th * c);   // d/dtheta
        const double dl = ul > 0.0 ? 0.5 * dul / sqrt(ul) * hp : 0.0, dr = ur > 0.0 ? 0.5 * dur / sqrt(ur) * hp : 0.0;
        gctl[i] = (float)(dl * sl + dr * sr);
    } else {
        const int b = i / T, t = i % T;
        double s = 0.0;
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < nseg; ++k) s += (double)partials[(((size_t)(b * 2 + c)) * nseg + k) * T + t];
        gctl[i] = (float)(s * 0.11512925464970228 * pow(10.0, (double)ctl[i] * 0.05));
    }
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline int st_check() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DASP_OK : (int)e;
}
inline bool st_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int st_nseg(long N) { return (int)((N + ST_SEG - 1) / ST_SEG); }
}  // namespace

extern "C" {

long dasp_stereo_partial_floats(int op, long B, int T, long N) {      // op 0 widener, 1 panner, 2 bus
    const long ns = st_nseg(N);
    return op == 0 ? B * ns : op == 1 ? B * T * ns * 2 : B * 2 * ns * T;
}

int dasp_widener_forward(const float* x, const float* width, float* y, int B, long N, void* stream) {
    if (!x || !width || !y || B <= 0 || N <= 0) return DASP_ERR_ARG;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(y);
    if ((long)B * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(widener_kernel<false>, dim3((unsigned)((long)B * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, width,
                       (const float*)nullptr, y, (float*)nullptr, N, nseg, vec);
    return st_check();
}
int dasp_widener_backward(const float* x, const float* width, const float* gy, float* gx, float* gwidth, float* partials, int B, long N,
                          void* stream) {
    if (!x || !width || !gy || !gx || !gwidth || !partials || B <= 0 || N <= 0) return DASP_ERR_ARG;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(gy) && st_al16(gx);
    if ((long)B * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(widener_kernel<true>, dim3((unsigned)((long)B * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, width, gy, gx,
                       partials, N, nseg, vec);
    hipLaunchKernelGGL(stereo_finalize_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, (const float*)partials, width, gwidth, B,
                       nseg, 1, 0);
    return st_check();
}

int dasp_panner_forward(const float* x, const float* pan, float* y, int B, int T, long N, void* stream) {
    if (!x || !pan || !y || B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(y);
    if ((long)B * T * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(panner_kernel<false>, dim3((unsigned)((long)B * T * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, pan,
                       (const float*)nullptr, y, (float*)nullptr, T, N, nseg, vec);
    return st_check();
}
int dasp_panner_backward(const float* x, const float* pan, const float* gy, float* gx, float* gpan, float* partials, int B, int T, long N,
                         void* stream) {
    if (!x || !pan || !gy || !gx || !gpan || !partials || B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(gy) && st_al16(gx);
    if ((long)B * T * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(panner_kernel<true>, dim3((unsigned)((long)B * T * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, pan, gy, gx,
                       partials, T, N, nseg, vec);
    hipLaunchKernelGGL(stereo_finalize_kernel, dim3((B * T + 127) / 128), dim3(128), 0, (hipStream_t)stream, (const float*)partials, pan, gpan,
                       B * T, nseg, T, 1);
    return st_check();
}

int dasp_bus_forward(const float* x, const float* send_db, float* y, int B, int T, long N, void* stream) {
    if (!x || !send_db || !y || B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    if (T > ST_TMAX) return DASP_ERR_UNSUPPORTED;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(y);
    if ((long)B * 2 * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(bus_kernel<false>, dim3((unsigned)((long)B * 2 * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, send_db,
                       (const float*)nullptr, y, (float*)nullptr, T, N, nseg, vec);
    return st_check();
}
int dasp_bus_backward(const float* x, const float* send_db, const float* gy, float* gx, float* gsend, float* partials, int B, int T, long N,
                      void* stream) {
    if (!x || !send_db || !gy || !gx || !gsend || !partials || B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    if (T > ST_TMAX) return DASP_ERR_UNSUPPORTED;
    const int nseg = st_nseg(N), vec = (N % 4 == 0) && st_al16(x) && st_al16(gy) && st_al16(gx);
    if ((long)B * 2 * nseg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(bus_kernel<true>, dim3((unsigned)((long)B * 2 * nseg)), dim3(ST_THREADS), 0, (hipStream_t)stream, x, send_db, gy, gx,
                       partials, T, N, nseg, vec);
    hipLaunchKernelGGL(stereo_finalize_kernel, dim3((B * T + 127) / 128), dim3(128), 0, (hipStream_t)stream, (const float*)partials, send_db,
                       gsend, B * T, nseg, T, 2);
    return st_check();
}

}  // extern "C"

// ================================================================================================
// stereo_mix: fader + pan + bus sum of T mono tracks in one pass - stereo_bus(stereo_panner(x, pan), gain_db) without the (B, 2, T, N)
// tensor between the two kernels, and an optional post-fader, post-pan effects send (a second bus, one more factor s per track).
//   mix[b, 0, n] = sum_t g l x[b, t, n],  mix[b, 1, n] = sum_t g r x[b, t, n],  send[b, c, n] = the same sums with s g in place of g
//   g = 10^(gain_db / 20), s = 10^(send_db / 20), l = sqrt(u_L), r = sqrt(u_R) the pan law of the panner above.
// A workgroup owns one segment of one item: `seg` samples (1024, 2048 or 4096: dasp_stereo_mix_segment) on seg / 16 threads, so a thread
// always owns MX_POS float4 positions, position j at sample (j * blockDim.x + threadIdx.x) * 4 of the segment. What is computed for a
// sample does not depend on the segment length; only the grouping of the backward pass's partial sums does.
namespace dasp {

constexpr int MX_TMAX = 256;     // tracks: 4 floats of coefficients and 16 floats of per-wave sums per track in LDS (20 KiB at the limit)
constexpr int MX_POS = 4;        // float4 positions per thread
constexpr int MX_SEG_MIN = 1024, MX_SEG_MAX = 4096;
constexpr int MX_WAVES = MX_SEG_MAX / (16 * 64);
constexpr int MX_UNROLL = 4;     // tracks whose loads are issued before the first of them is used

__device__ __forceinline__ f4 fma4(float a, f4 x, f4 acc) {       // explicit fmas: the same bits in every instantiation
    return f4{__builtin_fmaf(a, x.x, acc.x), __builtin_fmaf(a, x.y, acc.y), __builtin_fmaf(a, x.z, acc.z), __builtin_fmaf(a, x.w, acc.w)};
}
__device__ __forceinline__ float dot4_acc(f4 a, f4 b, float acc) {
    return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, acc))));
}

// pan law in fp64: l, r and (DERIV) their derivatives w.r.t. pan, zero where the gain itself is zero (stereo_finalize_kernel mode 1)
template <bool DERIV>
__device__ __forceinline__ void mix_pan(float pan, double& l, double& r, double& dl, double& dr) {
    const double hp = 1.57079632679489661923, ip = 2.0 / 3.14159265358979323846, th = (double)pan * hp, c = cos(th), sn = sin(th);
    const double ul = (hp - th) * ip * c, ur = th * ip * sn;
    l = sqrt(ul); r = sqrt(ur);
    if (DERIV) {
        const double dul = ip * (-c - (hp - th) * sn), dur = ip * (sn + th * c);       // d/dtheta
        dl = ul > 0.0 ? 0.5 * dul / l * hp : (ul != ul ? ul : 0.0);        // (a NaN pan is no hard pan: its gradient is NaN)
        dr = ur > 0.0 ? 0.5 * dur / r * hp : (ur != ur ? ur : 0.0);
    }
}

// coef[t] = g l, coef[MX_TMAX + t] = g r, and with SEND coef[2 MX_TMAX + t] = s g l, coef[3 MX_TMAX + t] = s g r: fp64, rounded once
template <bool SEND>
__device__ __forceinline__ void mix_coefs(float* coef, const float* __restrict__ gain_db, const float* __restrict__ pan,
                                          const float* __restrict__ send_db, int b, int T) {
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const size_t r0 = (size_t)b * T + t;
        double l, r, dl, dr;
        mix_pan<false>(pan[r0], l, r, dl, dr);
        const double g = pow(10.0, (double)gain_db[r0] * 0.05);
        coef[t] = (float)(g * l);
        coef[MX_TMAX + t] = (float)(g * r);
        if (SEND) {
            const double s = pow(10.0, (double)send_db[r0] * 0.05);
            coef[2 * MX_TMAX + t] = (float)(s * g * l);
            coef[3 * MX_TMAX + t] = (float)(s * g * r);
        }
    }
    __syncthreads();
}

// U tracks from t0 on at this thread's positions (zero past T and past N): U * MX_POS 16-byte loads in flight
template <bool STREAM, int U>
__device__ __forceinline__ void mix_load(f4 (&v)[U][MX_POS], const float* __restrict__ xb, int t0, int T, long N, const long (&pos)[MX_POS],
                                         int vec) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < MX_POS; ++j)
            v[u][j] = (t0 + u < T && pos[j] < N) ? ld4<STREAM>(xb + (size_t)(t0 + u) * N, pos[j], N, vec) : f4{0.f, 0.f, 0.f, 0.f};
}

template <bool SEND, int U>
__device__ __forceinline__ void mix_fwd_tracks(const float* coef, const f4 (&v)[U][MX_POS], int t0, int T, f4 (&aL)[MX_POS], f4 (&aR)[MX_POS],
                                               f4 (&sL)[MX_POS], f4 (&sR)[MX_POS]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t >= T) break;                           // uniform over the workgroup
        const float cl = coef[t], cr = coef[MX_TMAX + t];
        const float dl = SEND ? coef[2 * MX_TMAX + t] : 0.f, dr = SEND ? coef[3 * MX_TMAX + t] : 0.f;
#pragma unroll
        for (int j = 0; j < MX_POS; ++j) {
            aL[j] = fma4(cl, v[u][j], aL[j]); aR[j] = fma4(cr, v[u][j], aR[j]);
            if (SEND) { sL[j] = fma4(dl, v[u][j], sL[j]); sR[j] = fma4(dr, v[u][j], sR[j]); }
        }
    }
}

// The tracks go through two register buffers of MX_UNROLL tracks each: while one is accumulated the loads of the other are in flight, and
// the first buffer's loads are issued before the fp64 prologue. Every output sample is one chain of fmas over t = 0 .. T - 1.
template <bool SEND>
__global__ void __launch_bounds__(ST_THREADS)
mix_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gain_db, const float* __restrict__ pan, const float* __restrict__ send_db,
               float* __restrict__ mix, float* __restrict__ send, int T, long N, int seg, int nseg, int vec) {
    __shared__ float coef[(SEND ? 4 : 2) * MX_TMAX];
    constexpr int U = MX_UNROLL;
    const int b = blockIdx.x / nseg, sg = blockIdx.x % nseg;
    const float* xb = x + (size_t)b * T * N;
    long pos[MX_POS];
    f4 aL[MX_POS], aR[MX_POS], sL[MX_POS], sR[MX_POS];
#pragma unroll
    for (int j = 0; j < MX_POS; ++j) {
        pos[j] = (long)sg * seg + (long)(j * (int)blockDim.x + (int)threadIdx.x) * 4;
        aL[j] = aR[j] = sL[j] = sR[j] = f4{0.f, 0.f, 0.f, 0.f};
    }
    f4 va[U][MX_POS], vb[U][MX_POS];
    mix_load<false>(va, xb, 0, T, N, pos, vec);
    mix_coefs<SEND>(coef, gain_db, pan, send_db, b, T);
    for (int t0 = 0; t0 < T; t0 += 2 * U) {
        mix_load<false>(vb, xb, t0 + U, T, N, pos, vec);
        mix_fwd_tracks<SEND>(coef, va, t0, T, aL, aR, sL, sR);
        mix_load<false>(va, xb, t0 + 2 * U, T, N, pos, vec);
        mix_fwd_tracks<SEND>(coef, vb, t0 + U, T, aL, aR, sL, sR);
    }
    float* ml = mix + (size_t)b * 2 * N;
    float* sl = SEND ? send + (size_t)b * 2 * N : nullptr;
#pragma unroll
    for (int j = 0; j < MX_POS; ++j) {
        if (pos[j] >= N) continue;
        st4(ml, pos[j], N, vec, aL[j]); st4(ml + N, pos[j], N, vec, aR[j]);
        if (SEND) { st4(sl, pos[j], N, vec, sL[j]); st4(sl + N, pos[j], N, vec, sR[j]); }
    }
}

// gx of U tracks (GX) and their K dot products with the upstream rows, each reduced over the wave and parked at wsum[t][k][wave]
template <bool SEND, bool GX, int U>
__device__ __forceinline__ void mix_bwd_tracks(const float* coef, float* wsum, const f4 (&v)[U][MX_POS], const f4 (&g)[SEND ? 4 : 2][MX_POS],
                                               float* __restrict__ gxb, int t0, int T, long N, const long (&pos)[MX_POS], int vec) {
    constexpr int K = SEND ? 4 : 2;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t >= T) break;                           // uniform over the workgroup
        if (GX) {
            const float c0 = coef[t], c1 = coef[MX_TMAX + t];
            const float c2 = SEND ? coef[2 * MX_TMAX + t] : 0.f, c3 = SEND ? coef[3 * MX_TMAX + t] : 0.f;
#pragma unroll
            for (int j = 0; j < MX_POS; ++j) {
                if (pos[j] >= N) continue;
                f4 o = c1 * g[1][j];
                if (SEND) o = fma4(c2, g[2][j], fma4(c3, g[3][j], o));
                st4<true>(gxb + (size_t)t * N, pos[j], N, vec, fma4(c0, g[0][j], o));
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < MX_POS; ++j) a = dot4_acc(v[u][j], g[k][j], a);
            a = wave_sum(a);
            if (lane_id() == 0) wsum[(t * K + k) * MX_WAVES + wave_id()] = a;
        }
    }
}

// Backward: gx[b, t, n] = g l (gM[b, 0, n] + s gS[b, 0, n]) + g r (gM[b, 1, n] + s gS[b, 1, n]) and, per track, the dot products of x with the
// segment's gM (k = 0, 1) and gS (k = 2, 3) rows: partials[b][sg][t][k]. The upstream rows stay in registers over the loop across the
// tracks; every wave parks its sums in LDS at [t][k][wave] and ONE barrier per workgroup precedes the fixed-order sum over the waves.
template <bool SEND, bool GX>
__global__ void __launch_bounds__(ST_THREADS)
mix_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gain_db, const float* __restrict__ pan, const float* __restrict__ send_db,
               const float* __restrict__ gmix, const float* __restrict__ gsend, float* __restrict__ gx, float* __restrict__ partials, int T, long N,
               int seg, int nseg, int vec) {
    constexpr int K = SEND ? 4 : 2, U = 2;
    __shared__ float coef[(GX ? K : 1) * MX_TMAX];
    __shared__ float wsum[MX_TMAX * K * MX_WAVES];
    const int b = blockIdx.x / nseg, sg = blockIdx.x % nseg;
    const float* xb = x + (size_t)b * T * N;
    float* gxb = GX ? gx + (size_t)b * T * N : nullptr;
    const float* gm = gmix + (size_t)b * 2 * N;
    const float* gs = SEND ? gsend + (size_t)b * 2 * N : nullptr;
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    long pos[MX_POS];
    f4 g[K][MX_POS];
#pragma unroll
    for (int j = 0; j < MX_POS; ++j) {
        pos[j] = (long)sg * seg + (long)(j * (int)blockDim.x + (int)threadIdx.x) * 4;
        const bool in = pos[j] < N;
        g[0][j] = in ? ld4<true>(gm, pos[j], N, vec) : zero;
        g[1][j] = in ? ld4<true>(gm + N, pos[j], N, vec) : zero;
        if (SEND) {
            g[2][j] = in ? ld4<true>(gs, pos[j], N, vec) : zero;
            g[3][j] = in ? ld4<true>(gs + N, pos[j], N, vec) : zero;
        }
    }
    if (GX) mix_coefs<SEND>(coef, gain_db, pan, send_db, b, T);       // (the loads of g above are in flight under the fp64 prologue)
    for (int t0 = 0; t0 < T; t0 += U) {
        f4 v[U][MX_POS];
        mix_load<true>(v, xb, t0, T, N, pos, vec);
        mix_bwd_tracks<SEND, GX>(coef, wsum, v, g, gxb, t0, T, N, pos, vec);
    }
    __syncthreads();
    const int nw = blockDim.x >> 6;
    float* out = partials + ((size_t)b * nseg + sg) * T * K;
    for (int i = threadIdx.x; i < T * K; i += blockDim.x) {
        float s = wsum[i * MX_WAVES];
        for (int w = 1; w < nw; ++w) s += wsum[i * MX_WAVES + w];
        out[i] = s;
    }
}

// one wave per (b, t): lane l sums the partials of segments l, l + 64, ... in fp64 in index order, the 64 sums go through the fixed tree of
// wave_sum, and lane 0 applies the chain rule of the three controls in fp64 (one THREAD per (b, t) walked the segments one load latency
// after the other: the backward call at (1, 16, 262144), 256 segments, took 0.10 ms with it and takes 0.03 ms with this)
//   M_L = A_L + s S_L, M_R = A_R + s S_R;  d/dgain_db = c g (l M_L + r M_R);  d/dsend_db = c s g (l S_L + r S_R);  d/dpan = g (l' M_L + r' M_R)
constexpr int MX_FIN_WAVES = 4;
__global__ void __launch_bounds__(64 * MX_FIN_WAVES)
mix_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ gain_db, const float* __restrict__ pan,
                    const float* __restrict__ send_db, float* __restrict__ ggain, float* __restrict__ gpan, float* __restrict__ gsend_db, long BT,
                    int T, int nseg) {
    const long i = (long)blockIdx.x * MX_FIN_WAVES + wave_id();
    if (i >= BT) return;                                 // the whole wave leaves; there is no barrier below
    const long b = i / T;
    const int t = (int)(i % T), K = send_db ? 4 : 2;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int sg = lane_id(); sg < nseg; sg += 64) {
        const float* p = partials + (((size_t)b * nseg + sg) * T + t) * K;
        a[0] += (double)p[0]; a[1] += (double)p[1];
        if (send_db) { a[2] += (double)p[2]; a[3] += (double)p[3]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = wave_sum(a[k]);
    if (lane_id() != 0) return;
    double l, r, dl, dr;
    mix_pan<true>(pan[i], l, r, dl, dr);
    const double c = 0.11512925464970228, g = pow(10.0, (double)gain_db[i] * 0.05), s = send_db ? pow(10.0, (double)send_db[i] * 0.05) : 0.0;
    const double ml = a[0] + s * a[2], mr = a[1] + s * a[3];
    ggain[i] = (float)(c * g * (l * ml + r * mr));
    gpan[i] = (float)(g * (dl * ml + dr * mr));
    if (send_db) gsend_db[i] = (float)(c * s * g * (l * a[2] + r * a[3]));
}

}  // namespace dasp

namespace {
constexpr long MX_FILL = 2 * 256;        // workgroups below which a shorter segment is taken: two per CU of the 256
inline int mx_seg(long B, long N) {
    int seg = MX_SEG_MAX;
    while (seg > MX_SEG_MIN && B * ((N + seg - 1) / seg) < MX_FILL) seg >>= 1;
    return seg;
}
}  // namespace

extern "C" {

int dasp_stereo_mix_segment(long B, long N) { return B <= 0 || N <= 0 ? DASP_ERR_ARG : mx_seg(B, N); }
int dasp_stereo_mix_max_tracks(void) { return MX_TMAX; }
long dasp_stereo_mix_partial_floats(long B, int T, long N, int with_send) {
    if (B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    const long seg = mx_seg(B, N);
    return B * ((N + seg - 1) / seg) * T * (with_send ? 4 : 2);
}

int dasp_stereo_mix_forward(const float* x, const float* gain_db, const float* pan, const float* send_db, float* mix, float* send, int B, int T,
                            long N, void* stream) {
    if (!x || !gain_db || !pan || !mix || (send_db != nullptr) != (send != nullptr) || B <= 0 || T <= 0 || N <= 0) return DASP_ERR_ARG;
    if (T > MX_TMAX) return DASP_ERR_UNSUPPORTED;
    const int seg = mx_seg(B, N);
    const long ns = (N + seg - 1) / seg;
    if ((long)B * ns > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    const int nseg = (int)ns, vec = (N % 4 == 0) && st_al16(x) && st_al16(mix) && st_al16(send);
    const dim3 grid((unsigned)((long)B * nseg)), block(seg / (4 * MX_POS));
    if (send_db) hipLaunchKernelGGL(mix_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, x, gain_db, pan, send_db, mix, send, T, N, seg, nseg, vec);
    else hipLaunchKernelGGL(mix_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, x, gain_db, pan, send_db, mix, send, T, N, seg, nseg, vec);
    return st_check();
}

int dasp_stereo_mix_backward(const float* x, const float* gain_db, const float* pan, const float* send_db, const float* gmix, const float* gsend,
                             float* gx, float* ggain, float* gpan, float* gsend_db, float* partials, int B, int T, long N, void* stream) {
    if (!x || !gain_db || !pan || !gmix || !ggain || !gpan || !partials || (send_db != nullptr) != (gsend != nullptr) ||
        (send_db != nullptr) != (gsend_db != nullptr) || B <= 0 || T <= 0 || N <= 0)
        return DASP_ERR_ARG;
    if (T > MX_TMAX) return DASP_ERR_UNSUPPORTED;
    const int seg = mx_seg(B, N);
    const long ns = (N + seg - 1) / seg;
    if ((long)B * ns > 0x7fffffffL || (long)B * T > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    const int nseg = (int)ns, vec = (N % 4 == 0) && st_al16(x) && st_al16(gmix) && st_al16(gsend) && st_al16(gx);
    const dim3 grid((unsigned)((long)B * nseg)), block(seg / (4 * MX_POS));
    const hipStream_t st = (hipStream_t)stream;
#define DASP_MIX_BWD(SEND, GX) \
    hipLaunchKernelGGL((mix_bwd_kernel<SEND, GX>), grid, block, 0, st, x, gain_db, pan, send_db, gmix, gsend, gx, partials, T, N, seg, nseg, vec)
    if (send_db) { if (gx) DASP_MIX_BWD(true, true); else DASP_MIX_BWD(true, false); }
    else { if (gx) DASP_MIX_BWD(false, true); else DASP_MIX_BWD(false, false); }
#undef DASP_MIX_BWD
    const long BT = (long)B * T;
    hipLaunchKernelGGL(mix_finalize_kernel, dim3((unsigned)((BT + MX_FIN_WAVES - 1) / MX_FIN_WAVES)), dim3(64 * MX_FIN_WAVES), 0, st,
                       (const float*)partials, gain_db, pan, send_db, ggain, gpan, gsend_db, BT, T, nseg);
    return st_check();
}

}  // extern "C"
