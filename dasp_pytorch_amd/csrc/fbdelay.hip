// feedback_delay: echo / slap-back / comb resonator - one delay line read with Catmull-Rom interpolation whose output is fed back into it
// through a one-pole low-pass (the damping), mixed with the dry signal. A true recurrence, evaluated in place:
//
//   D = clamp(sr/1000 delay_ms, 2, sr/1000 max_delay_ms),  i = floor(D),  f = D - i          float64; f alone is rounded to float32
//   a = exp(-2 pi max(damping_hz, 0) / sr)                                                   float64, rounded to float32; +inf gives 0
//   r[n] = w_-1(f) v[n-i+1] + w_0(f) v[n-i] + w_1(f) v[n-i-1] + w_2(f) v[n-i-2]              (Catmull-Rom; v zero before sample 0)
//   w[n] = x[n] + feedback r[n],   v[n] = (1 - a) w[n] + a v[n-1],   y[n] = (1 - mix) x[n] + mix r[n]
// A NaN delay_ms: i = 2 before any address is formed and f stays NaN, so the item's y and gradients are NaN (an infinite one is clamped).
//
// The smallest lag is L = i - 1 >= 1: samples closer together than L do not depend on each other through the line, only through the
// one-pole. ONE WORKGROUP OWNS ONE (b, c) ROW and walks it in sequential steps of S = dasp_fbdelay_block(H, L) = min(L, 2048) samples.
// Inside a step a thread takes ceil(S / 256) | 1 consecutive samples (odd: the lanes' LDS words fall on distinct banks): the taps, w and y per sample, then v as a first-order scan with the
// constant ratio a - serially over the thread's samples, the threads' results combined across the lanes of a wave (six shifts) and
// across the four waves through LDS. Two barriers per step, which wait for LDS only. N / S steps are serial per row and a row occupies one CU: the op cannot fill
// the chip at training batch sizes (32 rows: 32 of 256 CUs), and a delay of two samples is one sample per step.
// The line's history is a ring of R = H + 2 + min(H - 1, 2048) floats of v in LDS, H = ceil(sr/1000 max_delay_ms) <=
// dasp_fbdelay_max_delay_samples() = 34816: a step reads back to n0 - i - 2 and writes up to n0 + S - 1, i + 2 + S <= R words. Behind it
// min(H - 1, 2048) words stage the step's y (gx in the backward kernel), so that global stores are one lane per consecutive sample.
// Dynamic LDS, up to 152 KiB.
// Forward traffic: x read, y written, and v written (bs, chs, N) when a gradient is wanted: 12 B per sample, 8 B with v = NULL.
//
// Backward, the same walk from the end of the row (m = N - 1 - n takes the place of n), with gr[n] = mix gy[n] + feedback gw[n]:
//   q[n] = sum_k w_k(f) gr[n+i+k] + a q[n+1],   gw[n] = (1 - a) q[n],   gx[n] = (1 - mix) gy[n] + gw[n]
// gr lives in the ring (zero past the end of the row), so gx is a gather and nothing is added atomically anywhere. r, w and the
// derivative taps are recomputed from the saved v, read from global memory; r and w come out bit for bit as in the forward pass. Both
// kernels load a step's inputs (x; gy, x and the saved v) into registers one step ahead, so that no step waits for memory. The sums
//   feedback: gw r,   mix: gy (r - x),   a: q (v[n-1] - w),   D: gr sum_k w'_k(f) v[n-i-k]   (nothing where D was clamped)
// are added per thread in float32 over the samples of one step and in float64 across the steps, then across the workgroup in a fixed
// order: four floats per row. A finalize kernel adds an item's channels in float64 and applies the chain rule (x sr/1000 for delay_ms,
// x -2 pi/sr a for damping_hz, zero where damping_hz < 0). Everything is bit-identical run to run and for an item alone or in a batch.
#include <atomic>

#include "row_helpers.hpp"

namespace dasp {

constexpr int FB_THREADS = 256;
constexpr int FB_BMAX = 2048;                        // longest step
constexpr int FB_SPT = 9;                            // most consecutive samples per thread and step: odd_spt<FB_THREADS>(FB_BMAX)
constexpr int FB_HMAX = 34816;                       // ring of 34816 + 2 + 2048 floats and 2048 of staging: 152 KiB of the workgroup's 160
constexpr int FB_NW = FB_THREADS / 64;

struct FbCfg { double k, sr, dmax; };                // k = sr / 1000 (samples per ms), dmax = k max_delay_ms
struct FbItem { int i; float f, a, fb, mix; bool inside; };

__host__ __device__ __forceinline__ int fb_block(int lag) { return lag < 1 ? 1 : (lag < FB_BMAX ? lag : FB_BMAX); }
__host__ __device__ __forceinline__ int fb_ring(int H) { return H + 2 + fb_block(H - 1); }

__device__ __forceinline__ FbItem fb_item(const float* __restrict__ ctl, int b, const FbCfg& g) {
    const float* q = ctl + (size_t)b * 4;
    const double raw = g.k * (double)q[0];
    const double D = raw < 2.0 ? 2.0 : (raw > g.dmax ? g.dmax : raw);      // a NaN stays
    const bool ok = D == D;
    const double fl = floor(D);
    FbItem it;
    it.i = ok ? (int)fl : 2;
    it.f = ok ? (float)(D - fl) : __builtin_nanf("");
    it.inside = !(raw < 2.0 || raw > g.dmax);                              // a NaN is not a clamped delay: it reaches the gradient
    it.a = (float)damping_pole((double)q[2], g.sr);
    it.fb = q[1];
    it.mix = q[3];
    return it;
}

// The scan of one step. `run`: the thread's last value of u[j] = in[j] + a u[j-1] taken over its own spt samples from zero; returns the
// value of u just before the thread's first sample. as = a^spt is a thread's ratio, alane = as^lane, carry = u before the step.
__device__ __forceinline__ float fb_scan(float run, float as, float alane, float carry, float* wtot) {
    const int lane = lane_id(), wv = wave_id();
    float agg = run, pw = as;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float t = shift_up(agg, d);
        if (lane >= d) agg = __builtin_fmaf(pw, t, agg);
        pw *= pw;
    }
    float excl = shift_up(agg, 1);
    if (lane == 0) excl = 0.f;
    if (lane == 63) wtot[wv] = agg;
    lds_barrier();
    float cw = carry;                                    // u before the wave's first sample; pw = as^64 is a wave's ratio
    for (int u = 0; u < wv; ++u) cw = __builtin_fmaf(pw, cw, wtot[u]);
    return __builtin_fmaf(alane, cw, excl);
}

// A step's inputs are loaded one step ahead into registers. The loads of a thread stand in a straight line behind ONE branch on the
// number of samples it takes (a branch around each load makes the compiler wait for each before the next is issued); addresses are
// held inside the row, and what lies past the step or the row is never used.
template <int K>
__device__ __forceinline__ void fb_load(float (&o)[FB_SPT], const float* __restrict__ p, long first, long N) {
#pragma unroll
    for (int s = 0; s < K; ++s) o[s] = p[min(first + s, N - 1)];
}
#define FB_BY_SPT(spt, CALL)                                                \
    switch (spt) {                                                          \
        case 1: { constexpr int K = 1; CALL; } break;                       \
        case 3: { constexpr int K = 3; CALL; } break;                       \
        case 5: { constexpr int K = 5; CALL; } break;                       \
        case 7: { constexpr int K = 7; CALL; } break;                       \
        default: { constexpr int K = FB_SPT; CALL; } break;                 \
    }

// backward: g[s], x[s], p[s] = gy, x, v[n - 1] at n = nh - s and h[u] = v[nh - i + 1 - u] (zero before the row)
struct FbBwdIn { float g[FB_SPT], x[FB_SPT], p[FB_SPT], h[FB_SPT + 3]; };
template <int K>
__device__ __forceinline__ void fb_load_bwd(FbBwdIn& o, const float* __restrict__ gr, const float* __restrict__ xr, const float* __restrict__ vr,
                                            long nh, int i, long N) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const long n = min(max(nh - s, 0L), N - 1);
        o.g[s] = gr[n];
        o.x[s] = xr[n];
        const float t = vr[max(n - 1, 0L)];
        o.p[s] = n > 0 ? t : 0.f;
    }
#pragma unroll
    for (int u = 0; u < K + 3; ++u) {
        const long j = nh - i + 1 - u;
        const float t = vr[min(max(j, 0L), N - 1)];
        o.h[u] = j >= 0 ? t : 0.f;
    }
}

template <bool SAVE>
__global__ void __launch_bounds__(FB_THREADS)
fbdelay_forward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, float* __restrict__ y, float* __restrict__ vout, long N, int C,
                       int H, const FbCfg g) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];        // the ring: v[n] at word n mod R
    __shared__ float wtot[2][FB_NW];
    __shared__ float last[2];                                             // v of the step's last sample
    const int row = blockIdx.x, tid = threadIdx.x, lane = lane_id();
    const FbItem it = fb_item(ctl, row / C, g);
    const int R = fb_ring(H), S = fb_block(it.i - 1), spt = odd_spt<FB_THREADS>(S), j0 = tid * spt;
    float* stage = fb_lds + R;                                            // the step's y, S words
    const CrW w = cr_weights(it.f);
    const float a = it.a, na = 1.f - a, fb = it.fb, mix = it.mix, dry = 1.f - mix;
    float as = 1.f;
    for (int s = 0; s < spt; ++s) as *= a;
    float alane = 1.f;
    for (int l = 0; l < lane; ++l) alane *= as;
    const float* xr = x + (size_t)row * N;
    float* yr = y + (size_t)row * N;
    float* vr = SAVE ? vout + (size_t)row * N : nullptr;

    for (int k = tid; k < R; k += FB_THREADS) fb_lds[k] = 0.f;
    if (tid < 2) last[tid] = 0.f;
    __syncthreads();

    float xn[FB_SPT] = {};                                                // x one step ahead
    FB_BY_SPT(spt, fb_load<K>(xn, xr, j0, N))
    int p0 = 0, par = 0;
    for (long n0 = 0; n0 < N; n0 += S) {
        const int Sc = (int)min((long)S, N - n0);
        const bool any = j0 < Sc;
        float tv[FB_SPT + 3], xv[FB_SPT], rv[FB_SPT], lv[FB_SPT];
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) xv[s] = xn[s];
        FB_BY_SPT(spt, fb_load<K>(xn, xr, n0 + S + j0, N))
        const int tb = p0 + j0 - it.i - 2;                                 // word of v[n - i - 2] of the thread's first sample
#pragma unroll
        for (int m = 0; m < FB_SPT + 3; ++m) tv[m] = fb_lds[ring_wrap(any ? tb + m : 0, R)];       // all of them, no branch: what is not needed is not used
        float run = 0.f;
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) {
            rv[s] = 0.f; lv[s] = 0.f;
            if (s < spt) {
                const bool act = j0 + s < Sc;
                float wn = 0.f;
                if (act) {
                    rv[s] = cr_dot(w, tv[s + 3], tv[s + 2], tv[s + 1], tv[s]);
                    wn = xv[s] + fb * rv[s];
                }
                run = act ? na * wn + a * run : a * run;                   // past the step's end: zero input, the same ratio
                lv[s] = run;
            }
        }
        const float cin = fb_scan(run, as, alane, last[par ^ 1], wtot[par]);
        float p = a;
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) {
            if (s < spt && j0 + s < Sc) {
                const float v = __builtin_fmaf(p, cin, lv[s]);
                fb_lds[ring_wrap(p0 + j0 + s, R)] = v;
                if (j0 + s == Sc - 1) last[par] = v;
                stage[j0 + s] = __builtin_fmaf(mix, rv[s], dry * xv[s]);
            }
            p *= a;
        }
        lds_barrier();
        // y and v leave through LDS, a lane per consecutive sample (a thread's own samples are spt words apart); the next step writes
        // `stage` behind its first barrier, which this thread reaches after these reads
        for (int j = tid; j < Sc; j += FB_THREADS) {
            st_stream(yr + n0 + j, stage[j]);
            if (SAVE) st_stream(vr + n0 + j, fb_lds[ring_wrap(p0 + j, R)]);
        }
        p0 += S;
        p0 -= p0 >= R ? R : 0;
        par ^= 1;
    }
}

__global__ void __launch_bounds__(FB_THREADS)
fbdelay_backward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ v, const float* __restrict__ gy,
                        float* __restrict__ gx, float* __restrict__ partials, long N, int C, int H, const FbCfg g) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];        // the ring: gr[N - 1 - m] at word m mod R
    __shared__ float wtot[2][FB_NW];
    __shared__ float last[2];                                             // q of the step's last sample
    __shared__ double red[FB_NW][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = lane_id();
    const FbItem it = fb_item(ctl, row / C, g);
    const int R = fb_ring(H), S = fb_block(it.i - 1), spt = odd_spt<FB_THREADS>(S), j0 = tid * spt;
    float* stage = fb_lds + R;                                            // the step's gx, S words
    const CrW w = cr_weights(it.f), dw = cr_dweights(it.f);
    const float a = it.a, na = 1.f - a, fb = it.fb, mix = it.mix, dry = 1.f - mix;
    float as = 1.f;
    for (int s = 0; s < spt; ++s) as *= a;
    float alane = 1.f;
    for (int l = 0; l < lane; ++l) alane *= as;
    const float* xr = x + (size_t)row * N;
    const float* vr = v + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;
    float* gxr = gx ? gx + (size_t)row * N : nullptr;

    for (int k = tid; k < R; k += FB_THREADS) fb_lds[k] = 0.f;
    if (tid < 2) last[tid] = 0.f;
    __syncthreads();

    FbBwdIn nx = {};                                                      // gy, x and the saved v one step ahead
    FB_BY_SPT(spt, fb_load_bwd<K>(nx, gr, xr, vr, N - 1 - j0, it.i, N))
    double s_fb = 0.0, s_mix = 0.0, s_a = 0.0, s_d = 0.0;
    int p0 = 0, par = 0;
    for (long m0 = 0; m0 < N; m0 += S) {
        const int Sc = (int)min((long)S, N - m0);
        const bool any = j0 < Sc;
        const long nh = N - 1 - m0 - j0;                                   // the thread's first sample: it walks down from here
        float tv[FB_SPT + 3], gv[FB_SPT], lv[FB_SPT], xv[FB_SPT], pv[FB_SPT], hv[FB_SPT + 3];
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) { gv[s] = nx.g[s]; xv[s] = nx.x[s]; pv[s] = nx.p[s]; }
#pragma unroll
        for (int u = 0; u < FB_SPT + 3; ++u) hv[u] = nx.h[u];
        FB_BY_SPT(spt, fb_load_bwd<K>(nx, gr, xr, vr, nh - S, it.i, N))
        const int tb = p0 + j0 - it.i - 2;                                 // word of gr[n + i + 2] of the thread's first sample
#pragma unroll
        for (int m = 0; m < FB_SPT + 3; ++m) tv[m] = fb_lds[ring_wrap(any ? tb + m : 0, R)];       // all of them, no branch: what is not needed is not used
        float run = 0.f;
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) {
            lv[s] = 0.f;
            if (s < spt) {
                const bool act = j0 + s < Sc;
                float sn = 0.f;
                if (act) {
                    sn = cr_dot(w, tv[s + 3], tv[s + 2], tv[s + 1], tv[s]);    // gr[n+i-1], gr[n+i], gr[n+i+1], gr[n+i+2]
                }
                run = act ? sn + a * run : a * run;
                lv[s] = run;
            }
        }
        const float cin = fb_scan(run, as, alane, last[par ^ 1], wtot[par]);
        float p = a, t_fb = 0.f, t_mix = 0.f, t_a = 0.f, t_d = 0.f;
#pragma unroll
        for (int s = 0; s < FB_SPT; ++s) {
            if (s < spt && j0 + s < Sc) {
                const float q = __builtin_fmaf(p, cin, lv[s]);
                const float gw = na * q;
                const float grn = __builtin_fmaf(fb, gw, mix * gv[s]);
                fb_lds[ring_wrap(p0 + j0 + s, R)] = grn;
                if (j0 + s == Sc - 1) last[par] = q;
                stage[j0 + s] = __builtin_fmaf(dry, gv[s], gw);
                const float xs = xv[s], vp = pv[s];
                const float r = cr_dot(w, hv[s], hv[s + 1], hv[s + 2], hv[s + 3]);
                const float dr = cr_dot(dw, hv[s], hv[s + 1], hv[s + 2], hv[s + 3]);
                const float wn = xs + fb * r;
                t_fb = __builtin_fmaf(gw, r, t_fb);
                t_mix = __builtin_fmaf(gv[s], r - xs, t_mix);
                t_a = __builtin_fmaf(q, vp - wn, t_a);
                t_d += it.inside ? grn * dr : 0.f;
            }
            p *= a;
        }
        s_fb += (double)t_fb; s_mix += (double)t_mix; s_a += (double)t_a; s_d += (double)t_d;
        lds_barrier();
        if (gxr)                                                           // gx leaves through LDS, as y does
            for (int j = tid; j < Sc; j += FB_THREADS) st_stream(gxr + (N - 1 - m0 - j), stage[j]);
        p0 += S;
        p0 -= p0 >= R ? R : 0;
        par ^= 1;
    }
    s_fb = wave_sum(s_fb); s_mix = wave_sum(s_mix); s_a = wave_sum(s_a); s_d = wave_sum(s_d);
    if (lane == 0) {
        double* r = red[wave_id()];
        r[0] = s_d; r[1] = s_fb; r[2] = s_a; r[3] = s_mix;
    }
    __syncthreads();
    if (tid < 4) {
        double sum = red[0][tid];
#pragma unroll
        for (int u = 1; u < FB_NW; ++u) sum += red[u][tid];
        partials[(size_t)row * 4 + tid] = (float)sum;
    }
}

// One thread per item: its channels' partials in fp64, channel by channel, then the chain rule to delay_ms and damping_hz.
__global__ void fbdelay_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ ctl, float* __restrict__ gctl, int B, int C,
                                        const FbCfg g) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const float* q = partials + ((size_t)b * C + c) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += (double)q[k];
    }
    const double damping = (double)ctl[(size_t)b * 4 + 2];
    float* o = gctl + (size_t)b * 4;
    o[0] = (float)(g.k * s[0]);
    o[1] = (float)s[1];
    o[2] = damping < 0.0 ? 0.f : (float)(-6.283185307179586 / g.sr * damping_pole(damping, g.sr) * s[2]);
    o[3] = (float)s[3];
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline bool fb_h_ok(int H) { return H >= 2 && H <= FB_HMAX; }
inline size_t fb_lds_bytes(int H) { return (size_t)(fb_ring(H) + fb_block(H - 1)) * sizeof(float); }       // the ring and the staged step

// The ring is more LDS than a kernel gets unasked (64 KiB): asked for once per device - by dasp_fbdelay_prepare() when the library is
// loaded, so that no call has to (a call may be under stream capture) - and by the first call on any other device.
int fb_prepare() {
    static std::atomic<bool> asked[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (dev >= 0 && dev < 64 && asked[dev].load(std::memory_order_acquire)) return DASP_OK;
    const int bytes = (int)fb_lds_bytes(FB_HMAX);
    for (const void* f : {reinterpret_cast<const void*>(fbdelay_forward_kernel<true>), reinterpret_cast<const void*>(fbdelay_forward_kernel<false>),
                          reinterpret_cast<const void*>(fbdelay_backward_kernel)}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
    }
    if (dev >= 0 && dev < 64) asked[dev].store(true, std::memory_order_release);
    return DASP_OK;
}

int fb_args(const float* x, const float* ctl, int B, int C, long N, int H, double sample_rate, double max_delay_ms) {
    if (!x || !ctl || B <= 0 || C <= 0 || N <= 0 || H < 2 || !(sample_rate > 0.0) || !(sample_rate - sample_rate == 0.0) ||
        !(sample_rate / 1000.0 * max_delay_ms >= 2.0) || !(sample_rate / 1000.0 * max_delay_ms <= (double)H))
        return DASP_ERR_ARG;
    if (!fb_h_ok(H) || (long)B * C > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
}  // namespace

extern "C" {

int dasp_fbdelay_max_delay_samples(void) { return FB_HMAX; }
int dasp_fbdelay_block(int H, long lag) {
    if (H < 2 || lag < 1 || lag > (long)H - 1) return DASP_ERR_ARG;
    return fb_h_ok(H) ? fb_block((int)lag) : DASP_ERR_UNSUPPORTED;
}
long dasp_fbdelay_partial_floats(long rows, long N, int H) {
    if (rows <= 0 || N <= 0 || H < 2) return DASP_ERR_ARG;
    return fb_h_ok(H) ? rows * 4 : DASP_ERR_UNSUPPORTED;
}
int dasp_fbdelay_prepare(void) { return fb_prepare(); }

int dasp_fbdelay_forward(const float* x, const float* ctl, float* y, float* v, int B, int C, long N, int H, double sample_rate, double max_delay_ms,
                         void* stream) {
    if (!y) return DASP_ERR_ARG;
    int s = fb_args(x, ctl, B, C, N, H, sample_rate, max_delay_ms);
    if (s != DASP_OK) return s;
    if ((s = fb_prepare()) != DASP_OK) return s;
    const FbCfg g{sample_rate / 1000.0, sample_rate, sample_rate / 1000.0 * max_delay_ms};
    const dim3 grid((unsigned)((long)B * C)), block(FB_THREADS);
    if (v) hipLaunchKernelGGL(fbdelay_forward_kernel<true>, grid, block, fb_lds_bytes(H), (hipStream_t)stream, x, ctl, y, v, N, C, H, g);
    else hipLaunchKernelGGL(fbdelay_forward_kernel<false>, grid, block, fb_lds_bytes(H), (hipStream_t)stream, x, ctl, y, v, N, C, H, g);
    return launch_status();
}

int dasp_fbdelay_backward(const float* x, const float* ctl, const float* v, const float* gy, float* gx, float* gctl, float* partials, int B, int C,
                          long N, int H, double sample_rate, double max_delay_ms, void* stream) {
    if (!v || !gy || !gctl || !partials) return DASP_ERR_ARG;
    int s = fb_args(x, ctl, B, C, N, H, sample_rate, max_delay_ms);
    if (s != DASP_OK) return s;
    if ((s = fb_prepare()) != DASP_OK) return s;
    const FbCfg g{sample_rate / 1000.0, sample_rate, sample_rate / 1000.0 * max_delay_ms};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fbdelay_backward_kernel, dim3((unsigned)((long)B * C)), dim3(FB_THREADS), fb_lds_bytes(H), st, x, ctl, v, gy, gx, partials, N, C,
                       H, g);
    if ((s = launch_status()) != DASP_OK) return s;
    hipLaunchKernelGGL(fbdelay_finalize_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, st, (const float*)partials, ctl, gctl, B, C, g);
    return launch_status();
}

}  // extern "C"
