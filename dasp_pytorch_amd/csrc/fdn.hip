// fdn_reverb: feedback delay network - K delay lines of whole lengths m_k, coupled through the Householder matrix I - (2/K) 1 1^T, each
// fed through a one-pole low-pass (the damping), mixed with the dry signal. A true recurrence, evaluated in place:
//
//   T = clamp(decay_s, 0.01, 100),  g_k = 10^(-3 m_k / (sr T))                               float64, rounded once to float32
//   a = exp(-2 pi max(damping_hz, 0) / sr)                                                   float64, rounded to float32; +inf gives 0
//   r_k[n] = v_k[n - m_k],  u_k[n] = g_k r_k[n]                                              (every v_k zero before sample 0)
//   w_k[n] = x[n] + u_k[n] - (2/K) sum_j u_j[n],   v_k[n] = (1 - a) w_k[n] + a v_k[n-1]
//   wet[n] = K^(-1/2) sum_k s_ck r_k[n],  s_ck = (-1)^(k c) (1 without decorrelate),   y[n] = (1 - mix) x[n] + mix wet[n]
// A NaN decay_s or damping_hz passes its clamp: g_k or a is NaN and so are the item's y and gradients. The line lengths come from the
// host and no sample or control ever forms an address.
//
// This is csrc/fbdelay.hip with K lines. The smallest lag is min_k m_k: samples closer together than that depend on each other through
// the one-poles only. ONE WORKGROUP OWNS ONE (b, c) ROW and walks it in sequential steps of S = dasp_fdn_block(K, min m_k) =
// min(min m_k, 1024) samples. Inside a step a thread takes ceil(S / 256) | 1 consecutive samples (odd: the lanes' LDS words fall on
// distinct banks). Three passes over the lines, each a loop over k:
//   1. r_k from the rings: sum_j u_j and wet, hence y (kept in registers)
//   2. w_k, then v_k as a first-order scan with the constant ratio a - serially over the thread's samples and across the lanes of a wave
//      (six shifts, the powers of a shared by all lines); the result, complete inside its wave, goes to ring k
//   -- barrier --
//   3. the carry of the earlier waves and of the step before is added to the thread's own ring words; y goes to the staging area
//   -- barrier --  y (and the v_k, straight from the rings) leave through LDS, one lane per consecutive sample.
// Two barriers per step for any K, both waiting for LDS only. N / S steps are serial per row and a row occupies one CU.
// Ring k holds m_k + S floats of v_k: a step reads back to n0 - m_k and writes up to n0 + S - 1. Behind the K rings S words stage y
// (gx in the backward kernel): sum m_k + (K + 1) S floats of dynamic LDS, at most 152 KiB. With the steps at their longest that leaves
// dasp_fdn_max_delay_sum(K) = 38912 - 1024 (K + 1) samples for the lines: 29696 at K = 8, 21504 at K = 16.
// Forward traffic: x read, y written, and the K line signals v (rows, K, N) written when a control wants a gradient: 8 + 4 K B a sample.
//
// Backward, the same network run backwards in time (m = N - 1 - n takes the place of n; the matrix is symmetric), rho_k in the rings:
//   lam_k[n] = a lam_k[n+1] + rho_k[n + m_k],   om_k[n] = (1 - a) lam_k[n]
//   rho_k[n] = K^(-1/2) s_ck mix gy[n] + g_k (om_k[n] - (2/K) sum_j om_j[n]),   gx[n] = (1 - mix) gy[n] + sum_k om_k[n]
// The scan comes first here and the matrix after it: pass A scans ring k read m_k back, pass B (behind the barrier) completes lam_k
// and adds up om, pass C forms rho_k and the sums. gx is a gather and nothing is added atomically anywhere. r, w and wet are recomputed
// from the saved v, read from global memory. The sums
//   g_k: r_k (om_k - (2/K) sum_j om_j),   a: sum_k lam_k (v_k[n-1] - w_k),   mix: gy (wet - x)
// are added per thread in float32 over the samples of one step and in float64 across the steps, then across the workgroup in a fixed
// order: 18 floats per row. A finalize kernel adds an item's channels in float64 and applies the chain rules (decay_s: sum_k g_k ln 10
// 3 m_k / (sr T^2), nothing where decay_s was clamped; damping_hz: -2 pi/sr a, nothing where damping_hz < 0 or +inf). Everything is
// bit-identical run to run, for an item alone or in a batch, and for channel 0 with or without decorrelate. With only x wanting a
// gradient there is no saved v: the backward kernel's other instantiation walks the same steps and writes gx alone, the same bits.
#include <atomic>

#include "row_helpers.hpp"

namespace dasp {

constexpr int FDN_THREADS = 256;
constexpr int FDN_KMAX = 16;                          // most lines
constexpr int FDN_CAP = 1024;                         // longest step
constexpr int FDN_SPT = 5;                            // most consecutive samples per thread and step: odd_spt<FDN_THREADS>(FDN_CAP)
constexpr int FDN_WORDS = 38912;                      // floats of dynamic LDS: 152 KiB of the workgroup's 160
constexpr int FDN_NW = FDN_THREADS / 64;
constexpr int FDN_PART = FDN_KMAX + 2;                // a row's sums: g_0 .. g_15, a, mix

struct FdnCfg { double sr; int K, S, odd; int m[FDN_KMAX]; };      // odd: 1 when odd channels alternate the lines' signs (decorrelate)

__host__ __device__ __forceinline__ int fdn_block(long shortest) { return shortest < 1 ? 1 : (shortest < FDN_CAP ? (int)shortest : FDN_CAP); }
__host__ __device__ __forceinline__ long fdn_max_sum(int K) { return (long)FDN_WORDS - (long)(K + 1) * FDN_CAP; }

__device__ __forceinline__ double fdn_decay(double decay_s) { return decay_s < 0.01 ? 0.01 : (decay_s > 100.0 ? 100.0 : decay_s); }       // a NaN stays
__device__ __forceinline__ double fdn_gain(int m, double sr, double T) { return pow(10.0, -3.0 * (double)m / (sr * T)); }
// the input of line k: x + u_k - (2/K) sum_j u_j, in one form for both directions
__device__ __forceinline__ float fdn_w(float x, float u, float su, float c2) { return __builtin_fmaf(-c2, su, x + u); }

// What a workgroup keeps about its lines, filled once from the launch's configuration.
struct FdnTab {
    int m[FDN_KMAX], off[FDN_KMAX], R[FDN_KMAX], pos[2][FDN_KMAX];        // length, first ring word, ring words, word of the step's first sample
    float g[FDN_KMAX], sgn[FDN_KMAX];                                     // g_k, s_ck
    float wtot[2][FDN_KMAX][FDN_NW], last[2][FDN_KMAX];                   // the waves' totals of a step; the scans' value at the step's last sample
};

__device__ __forceinline__ void fdn_setup(FdnTab& t, float* ring, const FdnCfg& g, const float* __restrict__ ctl, int b, int c, int words) {
    const int tid = threadIdx.x;
    const double T = fdn_decay((double)ctl[(size_t)b * 3]);
    int off = 0;
#pragma unroll
    for (int k = 0; k < FDN_KMAX; ++k) {
        if (k < g.K) {
            const int m = max(g.m[k], 1);
            if (tid == k) {
                t.m[k] = m; t.off[k] = off; t.R[k] = m + g.S; t.pos[0][k] = 0; t.pos[1][k] = 0;
                t.g[k] = (float)fdn_gain(m, g.sr, T);
                t.sgn[k] = (g.odd && (c & 1) && (k & 1)) ? -1.f : 1.f;
                t.last[0][k] = 0.f; t.last[1][k] = 0.f;
            }
            off += m + g.S;
        }
    }
    for (int k = tid; k < words; k += FDN_THREADS) ring[k] = 0.f;
    __syncthreads();
}

// The wave's part of the scan of one line. `run`: the thread's last value of u[j] = in[j] + a u[j-1] taken over its own spt samples from
// zero; returns the value that the earlier lanes of the wave leave just before the thread's first sample. as = a^spt is a thread's ratio.
__device__ __forceinline__ float fdn_wave_scan(float run, float as, float* wtot) {
    const int lane = lane_id();
    float agg = run, pw = as;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float t = shift_up(agg, d);
        if (lane >= d) agg = __builtin_fmaf(pw, t, agg);
        pw *= pw;
    }
    float excl = shift_up(agg, 1);
    if (lane == 0) excl = 0.f;
    if (lane == 63) wtot[wave_id()] = agg;
    return excl;
}
// the value that the earlier waves and the step before leave just before the wave's first sample; as64 = as^64 is a wave's ratio
__device__ __forceinline__ float fdn_wave_carry(float carry, float as64, const float* wtot) {
    float cw = carry;
    const int wv = wave_id();
    for (int u = 0; u < wv; ++u) cw = __builtin_fmaf(as64, cw, wtot[u]);
    return cw;
}

// A step's inputs are loaded one step ahead into registers, in a straight line behind ONE branch on the number of samples a thread
// takes; addresses are held inside the row, and what lies past the step or the row is never used. dir = +1 forward, -1 backward.
template <int Q>
__device__ __forceinline__ void fdn_load(float (&o)[FDN_SPT], const float* __restrict__ p, long first, long dir, long N) {
#pragma unroll
    for (int s = 0; s < Q; ++s) o[s] = p[min(max(first + dir * s, 0L), N - 1)];
}
#define FDN_BY_SPT(spt, CALL)                                               \
    switch (spt) {                                                          \
        case 1: { constexpr int Q = 1; CALL; } break;                       \
        case 3: { constexpr int Q = 3; CALL; } break;                       \
        default: { constexpr int Q = FDN_SPT; CALL; } break;                \
    }

template <bool SAVE>
__global__ void __launch_bounds__(FDN_THREADS)
fdn_forward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, float* __restrict__ y, float* __restrict__ vout, long N, int C,
                   int words, const FdnCfg g) {
    extern __shared__ __attribute__((aligned(16))) float fdn_lds[];       // ring k: v_k[n] at word off_k + n mod R_k; then the staged y
    __shared__ FdnTab t;
    const int row = blockIdx.x, tid = threadIdx.x, lane = lane_id();
    const int b = row / C, K = g.K, S = g.S, spt = odd_spt<FDN_THREADS>(S), j0 = tid * spt;
    fdn_setup(t, fdn_lds, g, ctl, b, row % C, words);
    float* stage = fdn_lds + (words - S);
    const float a = (float)damping_pole((double)ctl[(size_t)b * 3 + 1], g.sr), na = 1.f - a, mix = ctl[(size_t)b * 3 + 2], dry = 1.f - mix;
    const float c2 = (float)(2.0 / (double)K), kinv = (float)(1.0 / sqrt((double)K));
    float as = 1.f;
    for (int s = 0; s < spt; ++s) as *= a;
    float alane = 1.f;
    for (int l = 0; l < lane; ++l) alane *= as;
    float as64 = as;
#pragma unroll
    for (int d = 0; d < 6; ++d) as64 *= as64;
    float pw[FDN_SPT], pa[FDN_SPT];                                        // a^(s+1) and a^(s+1) as^lane
    {
        float p = a;
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s) { pw[s] = p; pa[s] = p * alane; p *= a; }
    }
    const float* xr = x + (size_t)row * N;
    float* yr = y + (size_t)row * N;

    float xn[FDN_SPT] = {};                                               // x one step ahead
    FDN_BY_SPT(spt, fdn_load<Q>(xn, xr, j0, 1, N))
    int par = 0;
    for (long n0 = 0; n0 < N; n0 += S) {
        const int Sc = (int)min((long)S, N - n0);
        const bool any = j0 < Sc;
        float xv[FDN_SPT], su[FDN_SPT], wa[FDN_SPT], yv[FDN_SPT];
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s) { xv[s] = xn[s]; su[s] = 0.f; wa[s] = 0.f; }
        FDN_BY_SPT(spt, fdn_load<Q>(xn, xr, n0 + S + j0, 1, N))
        // 1. sum_j u_j and wet
        for (int k = 0; k < K; ++k) {
            const int R = t.R[k], rb = any ? t.pos[par][k] + j0 - t.m[k] : 0;
            const float* ring = fdn_lds + t.off[k];
            const float gk = t.g[k], sg = t.sgn[k];
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                if (s < spt) {                                             // no branch on the lane: what is not needed is not used
                    const float r = ring[ring_wrap(rb + s, R)];
                    su[s] += gk * r;
                    wa[s] += sg * r;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s) yv[s] = __builtin_fmaf(mix, kinv * wa[s], dry * xv[s]);
        // 2. w_k and the scan of v_k inside the wave
        for (int k = 0; k < K; ++k) {
            const int R = t.R[k], rb = any ? t.pos[par][k] + j0 - t.m[k] : 0, wb = any ? t.pos[par][k] + j0 : 0;
            float* ring = fdn_lds + t.off[k];
            const float gk = t.g[k];
            float lv[FDN_SPT], run = 0.f;
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                lv[s] = 0.f;
                if (s < spt) {
                    const bool act = j0 + s < Sc;
                    const float wn = fdn_w(xv[s], gk * ring[ring_wrap(rb + s, R)], su[s], c2);
                    run = act ? na * wn + a * run : a * run;               // past the step's end: zero input, the same ratio
                    lv[s] = run;
                }
            }
            const float excl = fdn_wave_scan(run, as, t.wtot[par][k]);
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s)
                if (s < spt && j0 + s < Sc) ring[ring_wrap(wb + s, R)] = __builtin_fmaf(pw[s], excl, lv[s]);
        }
        lds_barrier();
        // 3. the carry of the earlier waves and of the step before
        for (int k = 0; k < K; ++k) {
            const int R = t.R[k], wb = any ? t.pos[par][k] + j0 : 0;
            float* ring = fdn_lds + t.off[k];
            const float cw = fdn_wave_carry(t.last[par ^ 1][k], as64, t.wtot[par][k]);
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                if (s < spt && j0 + s < Sc) {
                    const int iw = ring_wrap(wb + s, R);
                    const float v = __builtin_fmaf(pa[s], cw, ring[iw]);
                    ring[iw] = v;
                    if (j0 + s == Sc - 1) t.last[par][k] = v;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s)
            if (s < spt && j0 + s < Sc) stage[j0 + s] = yv[s];
        if (tid < K) t.pos[par ^ 1][tid] = ring_wrap(t.pos[par][tid] + S, t.R[tid]);
        lds_barrier();
        // y and the v_k leave through LDS, a lane per consecutive sample; the next step writes `stage` and these ring words behind its
        // first barrier, which this thread reaches after these reads
        for (int j = tid; j < Sc; j += FDN_THREADS) st_stream(yr + n0 + j, stage[j]);
        if (SAVE) {
            for (int k = 0; k < K; ++k) {
                const int R = t.R[k], p0 = t.pos[par][k];
                const float* ring = fdn_lds + t.off[k];
                float* vr = vout + ((size_t)row * K + k) * N + n0;
                for (int j = tid; j < Sc; j += FDN_THREADS) st_stream(vr + j, ring[ring_wrap(p0 + j, R)]);
            }
        }
        par ^= 1;
    }
}

// CTL: the controls' sums as well (they need the saved v); without, gx alone from the same walk, bit for bit
template <bool CTL>
__global__ void __launch_bounds__(FDN_THREADS)
fdn_backward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ v, const float* __restrict__ gy,
                    float* __restrict__ gx, float* __restrict__ partials, long N, int C, int words, const FdnCfg g) {
    extern __shared__ __attribute__((aligned(16))) float fdn_lds[];       // ring k: rho_k[N - 1 - m] at word off_k + m mod R_k; then the staged gx
    __shared__ FdnTab t;
    __shared__ double red[FDN_NW][FDN_PART];
    const int row = blockIdx.x, tid = threadIdx.x, lane = lane_id();
    const int b = row / C, K = g.K, S = g.S, spt = odd_spt<FDN_THREADS>(S), j0 = tid * spt;
    fdn_setup(t, fdn_lds, g, ctl, b, row % C, words);
    float* stage = fdn_lds + (words - S);
    const float a = (float)damping_pole((double)ctl[(size_t)b * 3 + 1], g.sr), na = 1.f - a, mix = ctl[(size_t)b * 3 + 2], dry = 1.f - mix;
    const float c2 = (float)(2.0 / (double)K), kinv = (float)(1.0 / sqrt((double)K));
    float as = 1.f;
    for (int s = 0; s < spt; ++s) as *= a;
    float alane = 1.f;
    for (int l = 0; l < lane; ++l) alane *= as;
    float as64 = as;
#pragma unroll
    for (int d = 0; d < 6; ++d) as64 *= as64;
    float pw[FDN_SPT], pa[FDN_SPT];
    {
        float p = a;
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s) { pw[s] = p; pa[s] = p * alane; p *= a; }
    }
    const float* xr = x + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;
    const float* vrow = CTL ? v + (size_t)row * K * N : nullptr;
    float* gxr = gx ? gx + (size_t)row * N : nullptr;

    float gn[FDN_SPT] = {}, xn[FDN_SPT] = {};                             // gy and x one step ahead
    FDN_BY_SPT(spt, (fdn_load<Q>(gn, gr, N - 1 - j0, -1, N), fdn_load<Q>(xn, xr, N - 1 - j0, -1, N)))
    double acc[FDN_KMAX] = {}, s_a = 0.0, s_mix = 0.0;
    int par = 0;
    for (long m0 = 0; m0 < N; m0 += S) {
        const int Sc = (int)min((long)S, N - m0);
        const bool any = j0 < Sc;
        const long nh = N - 1 - m0 - j0;                                   // the thread's first sample: it walks down from here
        float gv[FDN_SPT], xv[FDN_SPT], su[FDN_SPT], wa[FDN_SPT], so[FDN_SPT];
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s) { gv[s] = gn[s]; xv[s] = xn[s]; su[s] = 0.f; wa[s] = 0.f; so[s] = 0.f; }
        FDN_BY_SPT(spt, (fdn_load<Q>(gn, gr, nh - S, -1, N), fdn_load<Q>(xn, xr, nh - S, -1, N)))
        // sum_j u_j and wet from the saved v
        for (int k = 0; CTL && k < K; ++k) {
            const float* vk = vrow + (size_t)k * N;
            const long jb = nh - t.m[k];
            const float gk = t.g[k], sg = t.sgn[k];
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                if (s < spt) {
                    const long j = jb - s;
                    const float q = vk[min(max(j, 0L), N - 1)];
                    const float r = j >= 0 ? q : 0.f;
                    su[s] += gk * r;
                    wa[s] += sg * r;
                }
            }
        }
        float t_mix = 0.f, t_a = 0.f;
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s)
            if (s < spt && j0 + s < Sc) t_mix = __builtin_fmaf(gv[s], kinv * wa[s] - xv[s], t_mix);
        // A. the scan of lam_k inside the wave
        for (int k = 0; k < K; ++k) {
            const int R = t.R[k], rb = any ? t.pos[par][k] + j0 - t.m[k] : 0, wb = any ? t.pos[par][k] + j0 : 0;
            float* ring = fdn_lds + t.off[k];
            float lv[FDN_SPT], run = 0.f;
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                lv[s] = 0.f;
                if (s < spt) {
                    const bool act = j0 + s < Sc;
                    const float in = ring[ring_wrap(rb + s, R)];           // rho_k[n + m_k]
                    run = act ? in + a * run : a * run;
                    lv[s] = run;
                }
            }
            const float excl = fdn_wave_scan(run, as, t.wtot[par][k]);
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s)
                if (s < spt && j0 + s < Sc) ring[ring_wrap(wb + s, R)] = __builtin_fmaf(pw[s], excl, lv[s]);
        }
        lds_barrier();
        // B. lam_k complete, and sum_j om_j
        for (int k = 0; k < K; ++k) {
            const int R = t.R[k], wb = any ? t.pos[par][k] + j0 : 0;
            float* ring = fdn_lds + t.off[k];
            const float cw = fdn_wave_carry(t.last[par ^ 1][k], as64, t.wtot[par][k]);
#pragma unroll
            for (int s = 0; s < FDN_SPT; ++s) {
                if (s < spt && j0 + s < Sc) {
                    const int iw = ring_wrap(wb + s, R);
                    const float lam = __builtin_fmaf(pa[s], cw, ring[iw]);
                    ring[iw] = lam;
                    if (j0 + s == Sc - 1) t.last[par][k] = lam;
                    so[s] += na * lam;
                }
            }
        }
        // C. rho_k into the rings, and the sums; k is a constant in every copy of the body, so that acc[] stays in registers
#pragma unroll
        for (int k = 0; k < FDN_KMAX; ++k) {
            if (k < K) {
                const int R = t.R[k], wb = any ? t.pos[par][k] + j0 : 0;
                float* ring = fdn_lds + t.off[k];
                const float* vk = CTL ? vrow + (size_t)k * N : nullptr;
                const long jb = nh - t.m[k];
                const float gk = t.g[k], ck = kinv * t.sgn[k] * mix;
                float t_g = 0.f;
#pragma unroll
                for (int s = 0; s < FDN_SPT; ++s) {
                    if (s < spt && j0 + s < Sc) {
                        const int iw = ring_wrap(wb + s, R);
                        const float lam = ring[iw];
                        const float z = __builtin_fmaf(-c2, so[s], na * lam);
                        ring[iw] = __builtin_fmaf(gk, z, ck * gv[s]);
                        if (CTL) {
                            const long n = nh - s, j = jb - s;
                            const float q = vk[min(max(j, 0L), N - 1)], pq = vk[min(max(n - 1, 0L), N - 1)];
                            const float r = j >= 0 ? q : 0.f, vp = n > 0 ? pq : 0.f;
                            t_g = __builtin_fmaf(r, z, t_g);
                            t_a = __builtin_fmaf(lam, vp - fdn_w(xv[s], gk * r, su[s], c2), t_a);
                        }
                    }
                }
                acc[k] += (double)t_g;
            }
        }
        s_a += (double)t_a; s_mix += (double)t_mix;
#pragma unroll
        for (int s = 0; s < FDN_SPT; ++s)
            if (s < spt && j0 + s < Sc) stage[j0 + s] = __builtin_fmaf(dry, gv[s], so[s]);
        if (tid < K) t.pos[par ^ 1][tid] = ring_wrap(t.pos[par][tid] + S, t.R[tid]);
        lds_barrier();
        if (gxr)                                                           // gx leaves through LDS, as y does
            for (int j = tid; j < Sc; j += FDN_THREADS) st_stream(gxr + (N - 1 - m0 - j), stage[j]);
        par ^= 1;
    }
    if (!CTL) return;
    const int wv = wave_id();
#pragma unroll
    for (int k = 0; k < FDN_KMAX; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) red[wv][k] = s;
    }
    s_a = wave_sum(s_a); s_mix = wave_sum(s_mix);
    if (lane == 0) { red[wv][FDN_KMAX] = s_a; red[wv][FDN_KMAX + 1] = s_mix; }
    __syncthreads();
    if (tid < FDN_PART) {
        double sum = red[0][tid];
#pragma unroll
        for (int u = 1; u < FDN_NW; ++u) sum += red[u][tid];
        partials[(size_t)row * FDN_PART + tid] = (float)sum;
    }
}

// One thread per item: its channels' partials in fp64, channel by channel, then the chain rules to decay_s and damping_hz.
__global__ void fdn_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ ctl, float* __restrict__ gctl, int B, int C,
                                    const FdnCfg g) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double raw = (double)ctl[(size_t)b * 3], T = fdn_decay(raw), damping = (double)ctl[(size_t)b * 3 + 1];
    const float* p = partials + (size_t)b * C * FDN_PART;
    double gd = 0.0;
#pragma unroll
    for (int k = 0; k < FDN_KMAX; ++k) {
        if (k < g.K) {
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += (double)p[(size_t)c * FDN_PART + k];
            const int m = max(g.m[k], 1);
            gd += s * fdn_gain(m, g.sr, T) * (2.302585092994046 * 3.0 * (double)m / (g.sr * T * T));
        }
    }
    double sa = 0.0, sm = 0.0;
    for (int c = 0; c < C; ++c) {
        sa += (double)p[(size_t)c * FDN_PART + FDN_KMAX];
        sm += (double)p[(size_t)c * FDN_PART + FDN_KMAX + 1];
    }
    float* o = gctl + (size_t)b * 3;
    o[0] = (raw < 0.01 || raw > 100.0) ? 0.f : (float)gd;                  // a NaN is not a clamped value: it reaches the gradient
    o[1] = (damping < 0.0 || damping > 1.7976931348623157e308) ? 0.f : (float)(-6.283185307179586 / g.sr * damping_pole(damping, g.sr) * sa);
    o[2] = (float)sm;
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {

// The rings are more LDS than a kernel gets unasked (64 KiB): asked for once per device - by dasp_fdn_prepare() when the library is
// loaded, so that no call has to (a call may be under stream capture) - and by the first call on any other device.
int fdn_prepare() {
    static std::atomic<bool> asked[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (dev >= 0 && dev < 64 && asked[dev].load(std::memory_order_acquire)) return DASP_OK;
    const int bytes = FDN_WORDS * (int)sizeof(float);
    for (const void* f : {reinterpret_cast<const void*>(fdn_forward_kernel<true>), reinterpret_cast<const void*>(fdn_forward_kernel<false>),
                          reinterpret_cast<const void*>(fdn_backward_kernel<true>), reinterpret_cast<const void*>(fdn_backward_kernel<false>)}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
    }
    if (dev >= 0 && dev < 64) asked[dev].store(true, std::memory_order_release);
    return DASP_OK;
}

// checks everything a launch depends on and fills the configuration; `words`: floats of dynamic LDS
int fdn_args(const float* x, const float* ctl, const int* delays, int B, int C, long N, int K, double sample_rate, int decorrelate, FdnCfg& g,
             int& words) {
    if (!x || !ctl || !delays || B <= 0 || C <= 0 || N <= 0 || K < 1 || K > FDN_KMAX || !(sample_rate > 0.0) ||
        !(sample_rate - sample_rate == 0.0))
        return DASP_ERR_ARG;
    long sum = 0, shortest = 0x7fffffffL;
    for (int k = 0; k < K; ++k) {
        if (delays[k] < 1) return DASP_ERR_ARG;
        sum += delays[k];
        shortest = delays[k] < shortest ? delays[k] : shortest;
    }
    if (sum > fdn_max_sum(K) || (long)B * C > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    g.sr = sample_rate; g.K = K; g.S = fdn_block(shortest); g.odd = decorrelate ? 1 : 0;
    for (int k = 0; k < FDN_KMAX; ++k) g.m[k] = k < K ? delays[k] : 1;
    words = (int)sum + (K + 1) * g.S;                                      // <= FDN_WORDS, since S <= FDN_CAP
    return DASP_OK;
}
}  // namespace

extern "C" {

int dasp_fdn_max_lines(void) { return FDN_KMAX; }
int dasp_fdn_block(int K, long shortest) {
    if (K < 1 || K > FDN_KMAX || shortest < 1) return DASP_ERR_ARG;
    return (long)K * shortest > fdn_max_sum(K) ? DASP_ERR_UNSUPPORTED : fdn_block(shortest);
}
long dasp_fdn_max_delay_sum(int K) { return K < 1 || K > FDN_KMAX ? DASP_ERR_ARG : fdn_max_sum(K); }
long dasp_fdn_partial_floats(long rows) { return rows <= 0 ? DASP_ERR_ARG : rows * FDN_PART; }
int dasp_fdn_prepare(void) { return fdn_prepare(); }

int dasp_fdn_forward(const float* x, const float* ctl, const int* delays, float* y, float* v, int B, int C, long N, int K, double sample_rate,
                     int decorrelate, void* stream) {
    if (!y) return DASP_ERR_ARG;
    FdnCfg g;
    int words = 0;
    int s = fdn_args(x, ctl, delays, B, C, N, K, sample_rate, decorrelate, g, words);
    if (s != DASP_OK) return s;
    if ((s = fdn_prepare()) != DASP_OK) return s;
    const dim3 grid((unsigned)((long)B * C)), block(FDN_THREADS);
    const size_t lds = (size_t)words * sizeof(float);
    if (v) hipLaunchKernelGGL(fdn_forward_kernel<true>, grid, block, lds, (hipStream_t)stream, x, ctl, y, v, N, C, words, g);
    else hipLaunchKernelGGL(fdn_forward_kernel<false>, grid, block, lds, (hipStream_t)stream, x, ctl, y, v, N, C, words, g);
    return launch_status();
}

int dasp_fdn_backward(const float* x, const float* ctl, const int* delays, const float* v, const float* gy, float* gx, float* gctl, float* partials,
                      int B, int C, long N, int K, double sample_rate, int decorrelate, void* stream) {
    if (!gy || (v ? !gctl || !partials : !gx)) return DASP_ERR_ARG;
    FdnCfg g;
    int words = 0;
    int s = fdn_args(x, ctl, delays, B, C, N, K, sample_rate, decorrelate, g, words);
    if (s != DASP_OK) return s;
    if ((s = fdn_prepare()) != DASP_OK) return s;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)B * C)), block(FDN_THREADS);
    const size_t lds = (size_t)words * sizeof(float);
    if (!v) {                                                              // gx alone: no saved v, no sums, no second launch
        hipLaunchKernelGGL(fdn_backward_kernel<false>, grid, block, lds, st, x, ctl, v, gy, gx, partials, N, C, words, g);
        return launch_status();
    }
    hipLaunchKernelGGL(fdn_backward_kernel<true>, grid, block, lds, st, x, ctl, v, gy, gx, partials, N, C, words, g);
    if ((s = launch_status()) != DASP_OK) return s;
    hipLaunchKernelGGL(fdn_finalize_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, st, (const float*)partials, ctl, gctl, B, C, g);
    return launch_status();
}

}  // extern "C"
