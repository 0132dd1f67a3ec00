// modulated_delay: chorus / flanger / vibrato - V voices of a delay line whose length an LFO moves, read with Catmull-Rom interpolation
// and mixed with the dry signal, fused: forward 8 B of HBM traffic per sample (read x, write y) plus the halo, backward 12 B (read x and
// gy, write gx), whatever V is. Bound by vector-instruction issue (the float64 LFO and read position), not by HBM.
//
//   theta = 2 pi (rate_hz n / sr + phase + c stereo_spread)                      (c the channel; phase and stereo_spread in turns)
//   d     = clamp(sr/1000 (delay_ms + depth_ms sin theta), 0, sr/1000 max_delay_ms)          samples, float64
//   p = n - d,  i = floor(p),  f = p - i                                         float64; f alone is rounded to float32
//   tap_v[n] = w_-1(f) x[i-1] + w_0(f) x[i] + w_1(f) x[i+1] + w_2(f) x[i+2]      (Catmull-Rom; x zero outside [0, N))
//   y[n]  = (1 - mix) x[n] + (mix / V) sum_v tap_v[n]
// The position is float64 because one float32 ulp of a 1000-sample delay is 6e-5 samples: 7e-4 of the peak in y. Only theta needs the
// absolute n; p, i and f are formed relative to the tile's first sample t0, where n - t0 and d are both small.
// The LFO: a thread takes the samples t0 + tid + 256 m. It reduces the phase of its first sample modulo one turn and takes one float64
// sincospi there, then turns (sin, cos) by the fixed step of 256 samples with four float64 multiply-adds per sample; the step's sine and
// cosine are computed once per workgroup and voice. A thread makes at most (T + H) / 256 + 1 steps: the drift stays below 1e-14.
// Non-finite control: p is NaN or finite (d is clamped). Where it is NaN, i = n before any address is formed and f stays NaN.
//
// A workgroup owns T = dasp_moddelay_tile(H) samples of one (b, c) row, from t0 on; H = ceil(sr/1000 max_delay_ms) bounds d.
// Forward: x over [t0 - H - 1, t0 + T + 2) is staged in LDS (i - 1 >= t0 - H - 1 and i + 2 <= t0 + T + 1); every voice's four taps are LDS
// reads. The voices are the outer loop - one voice's LFO state in registers at a time, no array indexed by a run-time voice, no scratch -
// and a thread keeps the wet sum of its T / 256 samples in registers.
// Backward, one kernel in two passes over the same LDS:
//   A  control gradients over the owned n, x staged as in the forward pass and gy over the owned samples. With t = -sum_k w'_k(f) x[i+k]
//      (the derivative of the tap by d; zero where d was clamped), per (row, tile, voice) the four partials
//        sum gy t,  sum gy t sin theta,  sum gy t cos theta,  sum gy t cos theta (n - t0)
//      and per (row, tile) one for mix, sum gy ((1/V) sum_v tap_v - x). The factor n of the rate_hz gradient stays out of the float32 sum:
//      the finalize kernel adds t0 x the cos partial in float64.
//   B  gx[j] = (1 - mix) gy[j] + (mix / V) sum over (v, n, k) with i_v[n] + k = j of w_k gy[n] is a scatter: gy is staged over
//      [t0 - 3, t0 + T + H + 3) - one sample more on either side than the footprint needs - and every (v, n) adds its four products into
//      an LDS tile of the T owned gx; each gx word is then written once. No global atomics. A voice only visits the n that can reach
//      the tile, n - t0 in [floor(d_min) - 3, T + ceil(d_max) + 3) with d_min, d_max from delay_ms -+ |depth_ms|: T + the LFO's swing
//      instead of T + H per voice. Skipped when gx is not asked for.
//      The LDS adds are float atomics, so their ORDER VARIES between runs: gx is reproducible to rounding, not bit for bit. (Two n collide
//      on a word whenever the delay grows, p advancing by less than one per sample, so no schedule of the n is free of collisions.)
//   A finalize kernel adds the partials of an item over its channels and tiles in float64, in a fixed order, and applies the chain rule
//   through d: y and the control gradients are bit-identical run to run, and an item gives the same bits alone and inside a batch.
#include "row_helpers.hpp"

namespace dasp {

constexpr int MD_THREADS = 256;
constexpr int MD_VMAX = 8;
constexpr int MD_HMAX = 8192;                // largest H: backward LDS (2 T + H + 6 floats) stays at 48 KiB, three workgroups per CU
constexpr int MD_GPAD = 3;                   // staged gy before t0 (and past t0 + T + H)
constexpr int MD_PART = 4;                   // partials per voice

struct MdCfg { double k, sr, dmax, spread; };                // k = sr / 1000 (samples per ms), dmax = k max_delay_ms
struct MdVoice { double delay, depth, rate, phase; };
struct MdPos { int i; float f; bool inside; };              // i relative to t0; inside: d was not clamped

__device__ __forceinline__ MdVoice md_voice(const float* __restrict__ ctl, int b, int V, int v) {
    const float* q = ctl + ((size_t)b * V + v) * 4;
    return MdVoice{(double)q[0], (double)q[1], (double)q[2], (double)q[3]};
}

// (sin, cos) of theta at sample n: the phase in turns, reduced to [-1/2, 1/2] before the one sincospi
__device__ __forceinline__ void md_lfo(const MdVoice& vc, const MdCfg& g, long n, int ch, double& s, double& c) {
    const double turns = vc.rate * (double)n / g.sr + vc.phase + (double)ch * g.spread;
    sincospi(2.0 * (turns - rint(turns)), &s, &c);
}
__device__ __forceinline__ void md_step(const MdVoice& vc, const MdCfg& g, double& s, double& c) {
    const double turns = vc.rate * (double)MD_THREADS / g.sr;
    sincospi(2.0 * (turns - rint(turns)), &s, &c);
}
__device__ __forceinline__ void md_turn(double& s, double& c, double ss, double sc) {
    const double s1 = __builtin_fma(s, sc, c * ss), c1 = __builtin_fma(c, sc, -(s * ss));
    s = s1; c = c1;
}

__device__ __forceinline__ MdPos md_pos(int nrel, double sn, const MdVoice& vc, const MdCfg& g) {
    const double raw = g.k * (vc.delay + vc.depth * sn);
    const double d = raw < 0.0 ? 0.0 : (raw > g.dmax ? g.dmax : raw);       // a NaN stays
    const double p = (double)nrel - d, fl = floor(p);
    const bool ok = p == p;
    MdPos r;
    r.i = ok ? (int)fl : nrel;
    r.f = ok ? (float)(p - fl) : __builtin_nanf("");
    r.inside = !(raw < 0.0 || raw > g.dmax);               // a NaN is not a clamped sample: it reaches the gradients
    return r;
}

// word of x[i - 1] in the staged window that starts at t0 - H - 1; the bound holds by construction (0 <= d <= H) and is enforced all the same
__device__ __forceinline__ int md_word(int i, int H, int T) { return min(max(i + H, 0), T + H - 1); }

template <int TPT>
__global__ void __launch_bounds__(MD_THREADS)
moddelay_forward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ mix, float* __restrict__ y, long N,
                        int ntile, int C, int V, int H, const MdCfg g) {
    constexpr int T = MD_THREADS * TPT;
    extern __shared__ __attribute__((aligned(16))) float md_lds[];      // x over [t0 - H - 1, t0 + T + 2)
    __shared__ double step[2 * MD_VMAX];
    float* xs = md_lds;
    const int row = blockIdx.x / ntile, tile = blockIdx.x % ntile, tid = threadIdx.x;
    const int b = row / C, ch = row % C;
    const long t0 = (long)tile * T;
    const float* xr = x + (size_t)row * N;

    for (int i = tid; i < T + H + 3; i += MD_THREADS) {
        const long j = t0 - H - 1 + i;
        xs[i] = (j >= 0 && j < N) ? xr[j] : 0.f;
    }
    if (tid < V) {
        double s, c;
        md_step(md_voice(ctl, b, V, tid), g, s, c);
        step[2 * tid] = s;
        step[2 * tid + 1] = c;
    }
    __syncthreads();

    float wet[TPT];
#pragma unroll
    for (int m = 0; m < TPT; ++m) wet[m] = 0.f;
    for (int v = 0; v < V; ++v) {
        const MdVoice vc = md_voice(ctl, b, V, v);
        const double ss = step[2 * v], sc = step[2 * v + 1];
        double s, c;
        md_lfo(vc, g, t0 + tid, ch, s, c);
#pragma unroll
        for (int m = 0; m < TPT; ++m) {
            const MdPos p = md_pos(tid + MD_THREADS * m, s, vc, g);
            wet[m] += cr_dot(cr_weights(p.f), xs + md_word(p.i, H, T));
            md_turn(s, c, ss, sc);
        }
    }

    const float mx = mix[b], mv = mx / (float)V;
    float* yr = y + (size_t)row * N;
#pragma unroll
    for (int m = 0; m < TPT; ++m) {
        const int nrel = tid + MD_THREADS * m;
        if (t0 + nrel < N) st_stream(yr + t0 + nrel, __builtin_fmaf(mv, wet[m], (1.f - mx) * xs[nrel + H + 1]));
    }
}

template <int TPT>
__global__ void __launch_bounds__(MD_THREADS)
moddelay_backward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ mix, const float* __restrict__ gy,
                         float* __restrict__ gx, float* __restrict__ partials, long N, int ntile, int C, int V, int H, const MdCfg g) {
    constexpr int T = MD_THREADS * TPT, NW = MD_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float md_lds[];
    __shared__ double step[2 * MD_VMAX];
    __shared__ float red[NW][MD_PART * MD_VMAX + 1];
    float* buf = md_lds;                                 // pass A: x over [t0 - H - 1, t0 + T + 2); pass B: gy over [t0 - 3, t0 + T + H + 3)
    float* own = md_lds + T + H + 2 * MD_GPAD;           // pass A: gy over [t0, t0 + T); pass B: the gx sums
    const int row = blockIdx.x / ntile, tile = blockIdx.x % ntile, tid = threadIdx.x;
    const int b = row / C, ch = row % C;
    const long t0 = (long)tile * T;
    const float* xr = x + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;

    for (int i = tid; i < T + H + 3; i += MD_THREADS) {
        const long j = t0 - H - 1 + i;
        buf[i] = (j >= 0 && j < N) ? xr[j] : 0.f;
    }
    for (int i = tid; i < T; i += MD_THREADS) own[i] = t0 + i < N ? gr[t0 + i] : 0.f;
    if (tid < V) {
        double s, c;
        md_step(md_voice(ctl, b, V, tid), g, s, c);
        step[2 * tid] = s;
        step[2 * tid + 1] = c;
    }
    __syncthreads();

    // ---- pass A: the owned n; samples past the end of the row count for nothing (their taps may hold an inf: 0 x inf)
    float accm = 0.f, accx = 0.f;
    for (int v = 0; v < V; ++v) {
        const MdVoice vc = md_voice(ctl, b, V, v);
        const double ss = step[2 * v], sc = step[2 * v + 1];
        double s, c;
        md_lfo(vc, g, t0 + tid, ch, s, c);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
        for (int m = 0; m < TPT; ++m) {
            const int nrel = tid + MD_THREADS * m;
            const bool valid = t0 + nrel < N;
            const MdPos p = md_pos(nrel, s, vc, g);
            const float* xs = buf + md_word(p.i, H, T);
            const float gv = own[nrel];
            const float t = (valid && p.inside) ? -gv * cr_dot(cr_dweights(p.f), xs) : 0.f;
            const float tc = t * (float)c;
            a0 += t;
            a1 = __builtin_fmaf(t, (float)s, a1);
            a2 += tc;
            a3 = __builtin_fmaf(tc, (float)nrel, a3);
            accm += valid ? gv * cr_dot(cr_weights(p.f), xs) : 0.f;
            if (v == 0) accx += valid ? gv * buf[nrel + H + 1] : 0.f;
            md_turn(s, c, ss, sc);
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
        if (lane_id() == 0) {
            float* r = red[wave_id()] + MD_PART * v;
            r[0] = a0; r[1] = a1; r[2] = a2; r[3] = a3;
        }
    }
    const float am = wave_sum(accm / (float)V - accx);
    if (lane_id() == 0) red[wave_id()][MD_PART * V] = am;
    __syncthreads();                                     // red complete; every read of buf and own of pass A done
    if (tid < MD_PART * V + 1) {
        float sum = red[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) sum += red[w][tid];
        partials[((size_t)row * ntile + tile) * (MD_PART * V + 1) + tid] = sum;
    }
    if (!gx) return;

    // ---- pass B: the scatter into the owned gx
    for (int i = tid; i < T + H + 2 * MD_GPAD; i += MD_THREADS) {
        const long j = t0 - MD_GPAD + i;
        buf[i] = (j >= 0 && j < N) ? gr[j] : 0.f;
    }
    for (int i = tid; i < T; i += MD_THREADS) own[i] = 0.f;
    __syncthreads();
    for (int v = 0; v < V; ++v) {
        const MdVoice vc = md_voice(ctl, b, V, v);
        const double ss = step[2 * v], sc = step[2 * v + 1];
        // the n that can reach the tile: n - t0 - d in [-2, T + 1), one more on either side for the LFO's rounding
        double dlo = g.k * (vc.delay - fabs(vc.depth)), dhi = g.k * (vc.delay + fabs(vc.depth));
        dlo = dlo < 0.0 ? 0.0 : (dlo > g.dmax ? g.dmax : dlo);
        dhi = dhi < 0.0 ? 0.0 : (dhi > g.dmax ? g.dmax : dhi);
        if (!(dlo == dlo && dhi == dhi)) { dlo = 0.0; dhi = g.dmax; }
        const int nlo = max((int)floor(dlo) - MD_GPAD, -MD_GPAD), nhi = min(T + (int)ceil(dhi), T + H) + MD_GPAD;
        double s, c;
        md_lfo(vc, g, t0 + nlo + tid, ch, s, c);
        for (int nrel = nlo + tid; nrel < nhi; nrel += MD_THREADS) {
            const long n = t0 + nrel;
            if (n >= 0 && n < N) {
                const MdPos p = md_pos(nrel, s, vc, g);
                const CrW w = cr_weights(p.f);
                const float gv = buf[nrel + MD_GPAD];
                const int j = p.i - 1;
                if ((unsigned)j < (unsigned)T) __hip_atomic_fetch_add(own + j, w.a * gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((unsigned)(j + 1) < (unsigned)T) __hip_atomic_fetch_add(own + j + 1, w.b * gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((unsigned)(j + 2) < (unsigned)T) __hip_atomic_fetch_add(own + j + 2, w.c * gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((unsigned)(j + 3) < (unsigned)T) __hip_atomic_fetch_add(own + j + 3, w.d * gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            md_turn(s, c, ss, sc);
        }
    }
    __syncthreads();
    const float mx = mix[b], mv = mx / (float)V;
    float* gxr = gx + (size_t)row * N;
    for (int i = tid; i < T; i += MD_THREADS)
        if (t0 + i < N) st_stream(gxr + t0 + i, __builtin_fmaf(mv, own[i], (1.f - mx) * buf[i + MD_GPAD]));
}

// One thread per (item, voice) and one per item for mix: the partials of the item's channels and tiles in fp64, channel by channel and
// tile by tile, then the chain rule through d = k (delay_ms + depth_ms sin theta), theta = 2 pi (rate_hz n / sr + phase + ...).
__global__ void moddelay_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ ctl, const float* __restrict__ mix,
                                         float* __restrict__ gctl, float* __restrict__ gmix, int B, int C, int V, int ntile, int T, const MdCfg g) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * (V + 1)) return;
    const int b = (int)(idx / (V + 1)), v = (int)(idx % (V + 1)), P = MD_PART * V + 1;
    const float* p = partials + (size_t)b * C * ntile * P;
    if (v == V) {
        double sm = 0.0;
        for (long k = 0; k < (long)C * ntile; ++k) sm += (double)p[k * P + MD_PART * V];
        gmix[b] = (float)sm;
        return;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < ntile; ++t) {
            const float* q = p + ((size_t)c * ntile + t) * P + MD_PART * v;
            s0 += (double)q[0];
            s1 += (double)q[1];
            s2 += (double)q[2];
            s3 += (double)q[3] + (double)((long)t * T) * (double)q[2];
        }
    const double tau = 6.283185307179586, depth = (double)ctl[((size_t)b * V + v) * 4 + 1], scale = (double)mix[b] / V * g.k;
    float* o = gctl + ((size_t)b * V + v) * 4;
    o[0] = (float)(scale * s0);
    o[1] = (float)(scale * s1);
    o[2] = (float)(scale * depth * tau / g.sr * s3);
    o[3] = (float)(scale * depth * tau * s2);
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline bool md_h_ok(int H) { return H >= 1 && H <= MD_HMAX; }
inline int md_tile(int H) { return H <= MD_HMAX / 2 ? 4096 : 2048; }          // 2 T + H + 6 floats of backward LDS: 48 KiB at both ends
inline long md_ntile(long N, int H) { return (N + md_tile(H) - 1) / md_tile(H); }

template <bool BWD>
int md_launch(const float* x, const float* ctl, const float* mix, const float* gy, float* out, float* gctl, float* gmix, float* partials, int B,
              int C, long N, int V, int H, double sample_rate, double max_delay_ms, double stereo_spread, void* stream) {
    if (!x || !ctl || !mix || (!BWD && !out) || (BWD && (!gy || !gctl || !gmix || !partials)) || B <= 0 || C <= 0 || N <= 0 || V < 1 || H < 1 ||
        !(sample_rate > 0.0) || !(max_delay_ms >= 0.0) || !(sample_rate / 1000.0 * max_delay_ms <= (double)H) || !(stereo_spread - stereo_spread == 0.0))
        return DASP_ERR_ARG;
    if (V > MD_VMAX || !md_h_ok(H)) return DASP_ERR_UNSUPPORTED;
    const long rows = (long)B * C, nt = md_ntile(N, H);
    if (rows * nt > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    const int T = md_tile(H);
    const MdCfg g{sample_rate / 1000.0, sample_rate, sample_rate / 1000.0 * max_delay_ms, stereo_spread};
    const dim3 grid((unsigned)(rows * nt)), block(MD_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    if (!BWD) {
        const size_t lds = (size_t)(T + H + 3) * sizeof(float);
        if (T == 4096) hipLaunchKernelGGL(moddelay_forward_kernel<16>, grid, block, lds, st, x, ctl, mix, out, N, (int)nt, C, V, H, g);
        else hipLaunchKernelGGL(moddelay_forward_kernel<8>, grid, block, lds, st, x, ctl, mix, out, N, (int)nt, C, V, H, g);
        return launch_status();
    }
    const size_t lds = (size_t)(2 * T + H + 2 * MD_GPAD) * sizeof(float);
    if (T == 4096) hipLaunchKernelGGL(moddelay_backward_kernel<16>, grid, block, lds, st, x, ctl, mix, gy, out, partials, N, (int)nt, C, V, H, g);
    else hipLaunchKernelGGL(moddelay_backward_kernel<8>, grid, block, lds, st, x, ctl, mix, gy, out, partials, N, (int)nt, C, V, H, g);
    const int s = launch_status();
    if (s != DASP_OK) return s;
    const long nfin = (long)B * (V + 1);
    hipLaunchKernelGGL(moddelay_finalize_kernel, dim3((unsigned)((nfin + 127) / 128)), dim3(128), 0, st, (const float*)partials, ctl, mix, gctl, gmix,
                       B, C, V, (int)nt, T, g);
    return launch_status();
}
}  // namespace

extern "C" {

int dasp_moddelay_max_voices(void) { return MD_VMAX; }
int dasp_moddelay_max_delay_samples(void) { return MD_HMAX; }
int dasp_moddelay_tile(int H) { return H < 1 ? DASP_ERR_ARG : md_h_ok(H) ? md_tile(H) : DASP_ERR_UNSUPPORTED; }
long dasp_moddelay_partial_floats(long rows, long N, int V, int H) {
    if (rows <= 0 || N <= 0 || V < 1 || H < 1) return DASP_ERR_ARG;
    if (V > MD_VMAX || !md_h_ok(H)) return DASP_ERR_UNSUPPORTED;
    return rows * md_ntile(N, H) * (MD_PART * V + 1);
}

int dasp_moddelay_forward(const float* x, const float* ctl, const float* mix, float* y, int B, int C, long N, int V, int H, double sample_rate,
                          double max_delay_ms, double stereo_spread, void* stream) {
    return md_launch<false>(x, ctl, mix, nullptr, y, nullptr, nullptr, nullptr, B, C, N, V, H, sample_rate, max_delay_ms, stereo_spread, stream);
}
int dasp_moddelay_backward(const float* x, const float* ctl, const float* mix, const float* gy, float* gx, float* gctl, float* gmix, float* partials,
                           int B, int C, long N, int V, int H, double sample_rate, double max_delay_ms, double stereo_spread, void* stream) {
    return md_launch<true>(x, ctl, mix, gy, gx, gctl, gmix, partials, B, C, N, V, H, sample_rate, max_delay_ms, stereo_spread, stream);
}

}  // extern "C"
