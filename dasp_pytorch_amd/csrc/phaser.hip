// phaser: K first-order all-pass stages in series whose shared coefficient a sine LFO sweeps, mixed with the dry signal - the first
// recurrence of the library whose coefficient changes with every sample.
//
//   theta = 2 pi (rate_hz n / sr + phase + c stereo_spread)                      (c the channel; phase and stereo_spread in turns)
//   f[n]  = clamp(center_hz 2^(depth sin theta), sr/4096, 0.49 sr);   t = tan(pi f / sr);   a[n] = (t - 1) / (t + 1)
//   s_0 = x;   s_k[n] = a[n] (s_{k-1}[n] - s_k[n-1]) + s_{k-1}[n-1],  k = 1..K            (every state zero before sample 0)
//   y[n]  = (1 - mix) x[n] + mix s_K[n]
// The phase is taken in float64 and reduced to a turn in [-1/2, 1/2] before anything is rounded: sin, exp2, tan and all that follows
// are float32, the first three with the rounding of their arguments carried along to first order (ph_lfo). A NaN control passes the
// clamp (comparisons, not fmin / fmax) and makes the item NaN.
//
// A stage is s[n] = p[n] s[n-1] + u[n] with p[n] = -a[n] and u[n] = a[n] in[n] + in[n-1]: an associative scan over the pairs (p, u) with
// (p1, u1) then (p2, u2) = (p1 p2, u2 + p2 u1), and no constant ratio to shorten it. ONE WORKGROUP OWNS ONE (b, c) ROW and walks it in
// tiles of T = dasp_phaser_tile(K) = 2048 samples; thread tid takes the 8 consecutive samples from 8 tid on. Per tile a[n] is computed once
// and with it everything the stages share: the running products of p inside a thread, the products a scan step multiplies by (six per
// lane), the product of the lanes before a lane. A stage is then
//   1  the recurrence over the thread's samples from zero state: its outputs and the pair (product of p, last value);
//   2  the scan of the pairs over the lanes of a wave on DPP (row_shr 1, 2, 4, 8, row_bcast 15, 31: six multiply-adds, the products are
//      the shared ones) and over the four waves through LDS (one barrier, which waits for LDS only);
//   3  the fix-up of the thread's outputs with the state that comes in times the running product.
// Stage k + 1 starts from the fixed-up output of stage k; the state that comes into a thread's run of stage k is also the input before
// the run of stage k + 1. From tile to tile K floats are carried. x comes in and y goes out through LDS, a lane per consecutive sample
// on the global side (row stride 9 words on the LDS side: no bank conflicts either way); x is loaded one tile ahead.
// Forward traffic: x read, y written, 8 B per sample; with `states` K floats per tile more: s_k[t0 - 1] of every tile, all the backward
// pass needs beyond x.
//
// Backward, the same walk from the last tile. Phase 1 rebuilds the tile in forward time from the saved states exactly as the forward
// kernel does and leaves in LDS, a word per sample and row: a, d_k = s_{k-1}[n] - s_k[n-1] for every stage, s_K - x, and the three
// weights that take the gradient of a to center_hz, depth and theta (zero where f was clamped). Phase 2 is the mirrored scan in
// reverse time - thread r takes the run of thread 255 - r, last sample first, so that the same scan serves:
//   gs_K = mix gy;   lam_k[n] = gs_k[n] - a[n+1] lam_k[n+1];   gs_{k-1}[n] = a[n] lam_k[n] + lam_k[n+1];   ga[n] += lam_k[n] d_k[n]
//   gx = gs_0 + (1 - mix) gy;   gmix = sum gy (s_K - x)
// with lam_k of the later tile's first sample carried (K floats) and a[n+1] of a run's last sample read from its neighbour. With
// da/dt = 2 / (t + 1)^2, dt/df = (pi / sr)(1 + t^2) and e = 2^(depth sin theta), unclamped f = center_hz e:
//   center_hz: sum ga da/df e,   depth: ln 2 sum ga da/df f sin theta,   phase: 2 pi ln 2 depth sum ga da/df f cos theta,
//   rate_hz: the phase's sum with the factor n / sr inside (n relative to the tile in float32, the tile's first sample added in float64).
// The sums are float32 per thread and tile, float64 across the tiles and then across the workgroup in a fixed order: five floats per
// row. A finalize kernel adds an item's channels in float64. No atomics anywhere: every result is bit-identical run to run and for an
// item alone or in a batch.
// LDS: forward 18 KiB; backward (K + 4) rows of 8 KiB and 18 KiB of staging, 146 KiB at K = 12 - dynamic, the limit raised once per device.
#include <atomic>

#include "row_helpers.hpp"

namespace dasp {

constexpr int PH_THREADS = 256;
constexpr int PH_SPT = 8;                            // consecutive samples per thread
constexpr int PH_TILE = PH_THREADS * PH_SPT;
constexpr int PH_NW = PH_THREADS / 64;
constexpr int PH_KMAX = 12;
constexpr int PH_STAGE = PH_TILE + PH_TILE / PH_SPT; // a staged tile: sample i at word i + i / 8
constexpr int PH_PART = 5;                           // partials per row: rate_hz, center_hz, depth, phase, mix

struct PhCfg { double sr, spread, wk; float lo, hi; };                   // wk = pi / sr; lo, hi: the clamp of f
struct PhItem { double step, base; float center, depth, mix; };          // step = rate_hz / sr, base = phase + c stereo_spread: turns
struct PhLfo { float a, wc, wd, wt; };                                    // a and the weights of ga for center_hz, depth and theta

__device__ __forceinline__ PhItem ph_item(const float* __restrict__ ctl, int b, int ch, const PhCfg& g) {
    const float* q = ctl + (size_t)b * 5;
    return PhItem{(double)q[0] / g.sr, (double)q[3] + (double)ch * g.spread, q[1], q[2], q[4]};
}

template <bool GRAD>
__device__ __forceinline__ PhLfo ph_lfo(const PhItem& it, const PhCfg& g, long n) {
    const double turns = __builtin_fma(it.step, (double)n, it.base), fr = turns - rint(turns);
    // float32 functions, each with the rounding of its argument carried along to first order: what the turn loses when it is rounded
    // (3e-8 turns, which 20 octaves of depth turn into 3e-6 of f), the product depth sin theta, and pi f / sr in front of tan
    const float th = (float)fr, dth = 6.2831855f * (float)(fr - (double)th);
    float s0, c0;
    sincospif(2.f * th, &s0, &c0);
    const float s = __builtin_fmaf(dth, c0, s0), c = __builtin_fmaf(-dth, s0, c0);
    const float p = it.depth * s, e0 = exp2f(p);
    const float e = e0 * __builtin_fmaf(0.6931472f, __builtin_fmaf(it.depth, s, -p), 1.f), raw = it.center * e;      // (a product: e0 = inf stays inf)
    const float f = raw < g.lo ? g.lo : (raw > g.hi ? g.hi : raw);         // a NaN stays
    const double wd = g.wk * (double)f;
    const float w = (float)wd, t0 = tanf(w);
    const float t = __builtin_fmaf((float)(wd - (double)w), __builtin_fmaf(t0, t0, 1.f), t0), t1 = t + 1.f;
    PhLfo r;
    r.a = (t - 1.f) / t1;
    r.wc = r.wd = r.wt = 0.f;
    if (GRAD && !(raw < g.lo || raw > g.hi)) {                             // a NaN is not a clamped sample: it reaches the gradients
        const float dadf = 2.f / (t1 * t1) * ((float)g.wk * __builtin_fmaf(t, t, 1.f));
        r.wc = dadf * e;
        r.wd = dadf * f * s;
        r.wt = dadf * f * c;
    }
    return r;
}

// What the K scans of a tile share. q[j]: product of p over the thread's samples up to j. m[d]: product of p over the lanes that the
// lane's partial result covers before scan step d. ep: product over the lanes before this one in its wave. wp: over the whole wave.
struct PhShare { float q[PH_SPT], m[6], ep, wp; };

__device__ __forceinline__ void ph_share(PhShare& sh, const float (&p)[PH_SPT]) {
    float r = 1.f;
#pragma unroll
    for (int j = 0; j < PH_SPT; ++j) { r *= p[j]; sh.q[j] = r; }
    sh.m[0] = r; r *= dpp_or_one<0x111, 0xf>(r);       // row_shr:1
    sh.m[1] = r; r *= dpp_or_one<0x112, 0xf>(r);       // row_shr:2
    sh.m[2] = r; r *= dpp_or_one<0x114, 0xf>(r);       // row_shr:4
    sh.m[3] = r; r *= dpp_or_one<0x118, 0xf>(r);       // row_shr:8
    sh.m[4] = r; r *= dpp_or_one<0x142, 0xa>(r);       // row_bcast:15   rows 1, 3 after the row before them
    sh.m[5] = r; r *= dpp_or_one<0x143, 0xc>(r);       // row_bcast:31   rows 2, 3 after rows 0..1
    sh.wp = read_lane(r, 63);
    const float up = shift_up(r, 1);
    sh.ep = lane_id() == 0 ? 1.f : up;
}

// The scan of one stage. `run`: the last value of the thread's recurrence from zero state; carry: the state before the tile; wt: the
// stage's two floats per wave (value, product). Returns the state before the thread's first sample. One barrier.
__device__ __forceinline__ float ph_scan(float run, const PhShare& sh, float carry, float* wt) {
    const int lane = lane_id(), wv = wave_id();
    float agg = run;
    agg = __builtin_fmaf(sh.m[0], dpp_or_zero<0x111, 0xf>(agg), agg);
    agg = __builtin_fmaf(sh.m[1], dpp_or_zero<0x112, 0xf>(agg), agg);
    agg = __builtin_fmaf(sh.m[2], dpp_or_zero<0x114, 0xf>(agg), agg);
    agg = __builtin_fmaf(sh.m[3], dpp_or_zero<0x118, 0xf>(agg), agg);
    agg = __builtin_fmaf(sh.m[4], dpp_or_zero<0x142, 0xa>(agg), agg);
    agg = __builtin_fmaf(sh.m[5], dpp_or_zero<0x143, 0xc>(agg), agg);
    float excl = shift_up(agg, 1);
    if (lane == 0) excl = 0.f;
    if (lane == 63) { wt[2 * wv] = agg; wt[2 * wv + 1] = sh.wp; }
    lds_barrier();
    float cw = carry;                                    // the state before the wave's first sample
    for (int u = 0; u < wv; ++u) cw = __builtin_fmaf(wt[2 * u + 1], cw, wt[2 * u]);
    return __builtin_fmaf(sh.ep, cw, excl);
}

// One stage over the thread's samples, forward time. cur: the stage's input, replaced by its output; cprev: the input before the first
// sample; carry: the stage's state before the tile. Returns the stage's state before the first sample, which is the next stage's cprev.
// KEEP: d[j] = in[j] - out[j-1], what the gradient of a[j] is taken against.
template <bool KEEP>
__device__ __forceinline__ float ph_stage(float (&cur)[PH_SPT], float (&d)[PH_SPT], const float (&a)[PH_SPT], const PhShare& sh, float cprev, float carry,
                                          float* wt) {
    float loc[PH_SPT], r = 0.f, ip = cprev;
#pragma unroll
    for (int j = 0; j < PH_SPT; ++j) {
        const float u = __builtin_fmaf(a[j], cur[j], ip);
        r = __builtin_fmaf(-a[j], r, u);
        loc[j] = r;
        ip = cur[j];
    }
    const float c = ph_scan(r, sh, carry, wt);
    float po = c;
#pragma unroll
    for (int j = 0; j < PH_SPT; ++j) {
        const float o = __builtin_fmaf(sh.q[j], c, loc[j]);
        if (KEEP) d[j] = cur[j] - po;
        po = o;
        cur[j] = o;
    }
    return c;
}

// x of a tile, a lane per consecutive sample, one tile ahead of its use; what lies past the row is zero. h: x before the tile (thread 0).
// (The loop is stage_load's, written out: as a call to it the kernels compile to other code, see row_helpers.hpp's rule.)
__device__ __forceinline__ void ph_load(float (&o)[PH_SPT], float& h, const float* __restrict__ p, long t0, long N, int tid) {
    const bool live = t0 >= 0 && t0 < N;
#pragma unroll
    for (int m = 0; m < PH_SPT; ++m) {
        const long n = t0 + tid + PH_THREADS * m;
        const float v = p[live ? min(n, N - 1) : 0];
        o[m] = live && n < N ? v : 0.f;
    }
    const float v = p[live && t0 > 0 ? t0 - 1 : 0];
    h = live && t0 > 0 ? v : 0.f;
}

template <bool SAVE>
__global__ void __launch_bounds__(PH_THREADS)
phaser_forward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, float* __restrict__ y, float* __restrict__ states, long N, int ntile,
                      int C, int K, const PhCfg g) {
    __shared__ float xs[PH_STAGE], ys[PH_STAGE];
    __shared__ float wt[2][2 * PH_NW];
    __shared__ float carry[2][PH_KMAX];
    __shared__ float halo;
    const int row = blockIdx.x, tid = threadIdx.x;
    const PhItem it = ph_item(ctl, row / C, row % C, g);
    const float mix = it.mix, dry = 1.f - mix;
    const float* xr = x + (size_t)row * N;
    float* yr = y + (size_t)row * N;
    float* sr = SAVE ? states + (size_t)row * ntile * K : nullptr;

    if (tid < K) {
        carry[0][tid] = 0.f;
        if (SAVE) sr[tid] = 0.f;                         // the states before the row
    }
    float xn[PH_SPT], hn;
    ph_load(xn, hn, xr, 0, N, tid);
    int par = 0, sc = 0;
    for (int ti = 0; ti < ntile; ++ti) {
        const long t0 = (long)ti * PH_TILE;
        stage_put<PH_SPT, PH_THREADS>(xs, xn, tid);
        if (tid == 0) halo = hn;
        ph_load(xn, hn, xr, t0 + PH_TILE, N, tid);
        lds_barrier();

        float cur[PH_SPT], a[PH_SPT], p[PH_SPT], none[PH_SPT];
        const int i0 = tid * PH_SPT;
#pragma unroll
        for (int j = 0; j < PH_SPT; ++j) {
            cur[j] = xs[stage_word<PH_SPT>(i0 + j)];
            a[j] = t0 + i0 + j < N ? ph_lfo<false>(it, g, t0 + i0 + j).a : 0.f;
            p[j] = -a[j];
        }
        float cprev = tid ? xs[stage_word<PH_SPT>(i0 - 1)] : halo;
        PhShare sh;
        ph_share(sh, p);
        const bool more = ti + 1 < ntile;
        for (int k = 0; k < K; ++k, sc ^= 1) {
            cprev = ph_stage<false>(cur, none, a, sh, cprev, carry[par][k], wt[sc]);
            if (tid == PH_THREADS - 1) {
                carry[par ^ 1][k] = cur[PH_SPT - 1];
                if (SAVE && more) sr[(size_t)(ti + 1) * K + k] = cur[PH_SPT - 1];
            }
        }
#pragma unroll
        for (int j = 0; j < PH_SPT; ++j) ys[stage_word<PH_SPT>(i0 + j)] = __builtin_fmaf(mix, cur[j], dry * xs[stage_word<PH_SPT>(i0 + j)]);
        lds_barrier();
        const int Tc = (int)min((long)PH_TILE, N - t0);
        for (int i = tid; i < Tc; i += PH_THREADS) st_stream(yr + t0 + i, ys[stage_word<PH_SPT>(i)]);
        par ^= 1;
    }
}

__global__ void __launch_bounds__(PH_THREADS)
phaser_backward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ states, const float* __restrict__ gy,
                       float* __restrict__ gx, float* __restrict__ partials, long N, int ntile, int C, int K, const PhCfg g) {
    extern __shared__ __attribute__((aligned(16))) float ph_lds[];        // K + 4 rows of a tile: sample 8 f + j at word 256 j + f
    __shared__ float s1[PH_STAGE], s2[PH_STAGE];                          // x, then gy | s_K - x, then gx
    __shared__ float wt[2][2 * PH_NW];
    __shared__ float cst[PH_KMAX], clam[2][PH_KMAX], anext[2];
    __shared__ float halo;
    __shared__ double red[PH_NW][PH_PART];
    float* rowA = ph_lds;
    float* rowC = ph_lds + PH_TILE;
    float* rowD = ph_lds + 2 * PH_TILE;
    float* rowT = ph_lds + 3 * PH_TILE;
    float* rowK = ph_lds + 4 * PH_TILE;                                   // d_1 .. d_K
    const int row = blockIdx.x, tid = threadIdx.x;
    const PhItem it = ph_item(ctl, row / C, row % C, g);
    const float mix = it.mix, dry = 1.f - mix;
    const float* xr = x + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;
    const float* sr = states + (size_t)row * ntile * K;
    float* gxr = gx ? gx + (size_t)row * N : nullptr;

    if (tid < K) clam[0][tid] = 0.f;
    if (tid == 0) anext[0] = 0.f;
    float xn[PH_SPT], gn[PH_SPT], hn, unused;
    ph_load(xn, hn, xr, (long)(ntile - 1) * PH_TILE, N, tid);
    ph_load(gn, unused, gr, (long)(ntile - 1) * PH_TILE, N, tid);
    double s_rate = 0.0, s_center = 0.0, s_depth = 0.0, s_phase = 0.0, s_mix = 0.0;
    int par = 0, sc = 0;
    for (int ti = ntile - 1; ti >= 0; --ti) {
        const long t0 = (long)ti * PH_TILE;
        float gv[PH_SPT];
        stage_put<PH_SPT, PH_THREADS>(s1, xn, tid);
        if (tid == 0) halo = hn;
        if (tid < K) cst[tid] = ti ? sr[(size_t)ti * K + tid] : 0.f;
#pragma unroll
        for (int m = 0; m < PH_SPT; ++m) gv[m] = gn[m];
        ph_load(xn, hn, xr, t0 - PH_TILE, N, tid);
        ph_load(gn, unused, gr, t0 - PH_TILE, N, tid);
        lds_barrier();

        // ---- phase 1, forward time: thread tid has the samples 8 tid + j
        {
            float cur[PH_SPT], x0[PH_SPT], a[PH_SPT], p[PH_SPT], d[PH_SPT];
            const int i0 = tid * PH_SPT;
#pragma unroll
            for (int j = 0; j < PH_SPT; ++j) {
                x0[j] = cur[j] = s1[stage_word<PH_SPT>(i0 + j)];
                PhLfo l{0.f, 0.f, 0.f, 0.f};
                if (t0 + i0 + j < N) l = ph_lfo<true>(it, g, t0 + i0 + j);
                a[j] = l.a;
                p[j] = -a[j];
                const int wd = PH_THREADS * j + tid;
                rowA[wd] = l.a; rowC[wd] = l.wc; rowD[wd] = l.wd; rowT[wd] = l.wt;
            }
            float cprev = tid ? s1[stage_word<PH_SPT>(i0 - 1)] : halo;
            PhShare sh;
            ph_share(sh, p);
            for (int k = 0; k < K; ++k, sc ^= 1) {
                cprev = ph_stage<true>(cur, d, a, sh, cprev, cst[k], wt[sc]);
#pragma unroll
                for (int j = 0; j < PH_SPT; ++j) rowK[(size_t)k * PH_TILE + PH_THREADS * j + tid] = d[j];
            }
#pragma unroll
            for (int j = 0; j < PH_SPT; ++j) s2[stage_word<PH_SPT>(i0 + j)] = cur[j] - x0[j];
        }
        stage_put<PH_SPT, PH_THREADS>(s1, gv, tid);                             // every thread read its x before the barrier of the first stage
        lds_barrier();

        // ---- phase 2, reverse time: thread tid has the run of thread f = 255 - tid; m = 0 is its last sample, j = 7 - m
        {
            const int f = PH_THREADS - 1 - tid, i0 = f * PH_SPT;
            float gs[PH_SPT], gq[PH_SPT], a[PH_SPT], p[PH_SPT], ga[PH_SPT], loc[PH_SPT];
            float t_mix = 0.f;
#pragma unroll
            for (int m = 0; m < PH_SPT; ++m) {
                const int j = PH_SPT - 1 - m;
                gq[m] = s1[stage_word<PH_SPT>(i0 + j)];
                t_mix = __builtin_fmaf(gq[m], t0 + i0 + j < N ? s2[stage_word<PH_SPT>(i0 + j)] : 0.f, t_mix);
                gs[m] = mix * gq[m];
                a[m] = rowA[PH_THREADS * j + f];
                ga[m] = 0.f;
            }
            p[0] = -(tid ? rowA[f + 1] : anext[par]);    // a of the sample after the run's last
#pragma unroll
            for (int m = 1; m < PH_SPT; ++m) p[m] = -a[m - 1];
            PhShare sh;
            ph_share(sh, p);
            for (int k = K - 1; k >= 0; --k, sc ^= 1) {
                float r = 0.f;
#pragma unroll
                for (int m = 0; m < PH_SPT; ++m) { r = __builtin_fmaf(p[m], r, gs[m]); loc[m] = r; }
                const float c = ph_scan(r, sh, clam[par][k], wt[sc]);
                float later = c;
#pragma unroll
                for (int m = 0; m < PH_SPT; ++m) {
                    const float lam = __builtin_fmaf(sh.q[m], c, loc[m]);
                    ga[m] = __builtin_fmaf(lam, rowK[(size_t)k * PH_TILE + PH_THREADS * (PH_SPT - 1 - m) + f], ga[m]);
                    gs[m] = __builtin_fmaf(a[m], lam, later);
                    later = lam;
                }
                if (tid == PH_THREADS - 1) clam[par ^ 1][k] = later;
            }
            if (tid == PH_THREADS - 1) anext[par ^ 1] = a[PH_SPT - 1];
            float t_c = 0.f, t_d = 0.f, t_t = 0.f, t_r = 0.f;
#pragma unroll
            for (int m = 0; m < PH_SPT; ++m) {
                const int j = PH_SPT - 1 - m, wd = PH_THREADS * j + f;
                const bool valid = t0 + i0 + j < N;
                s2[stage_word<PH_SPT>(i0 + j)] = __builtin_fmaf(dry, gq[m], gs[m]);
                const float wc = rowC[wd], wdp = rowD[wd], wth = rowT[wd];
                const float tt = valid ? ga[m] * wth : 0.f;
                t_c += valid ? ga[m] * wc : 0.f;
                t_d += valid ? ga[m] * wdp : 0.f;
                t_t += tt;
                t_r = __builtin_fmaf(tt, (float)(i0 + j), t_r);
            }
            s_center += (double)t_c; s_depth += (double)t_d; s_phase += (double)t_t; s_mix += (double)t_mix;
            s_rate += (double)t_r + (double)t0 * (double)t_t;
        }
        lds_barrier();
        if (gxr) {
            const int Tc = (int)min((long)PH_TILE, N - t0);
            for (int i = tid; i < Tc; i += PH_THREADS) st_stream(gxr + t0 + i, s2[stage_word<PH_SPT>(i)]);
        }
        par ^= 1;
    }
    s_rate = wave_sum(s_rate); s_center = wave_sum(s_center); s_depth = wave_sum(s_depth); s_phase = wave_sum(s_phase); s_mix = wave_sum(s_mix);
    if (lane_id() == 0) {
        double* r = red[wave_id()];
        r[0] = s_rate; r[1] = s_center; r[2] = s_depth; r[3] = s_phase; r[4] = s_mix;
    }
    __syncthreads();
    if (tid < PH_PART) {
        double sum = red[0][tid];
#pragma unroll
        for (int u = 1; u < PH_NW; ++u) sum += red[u][tid];
        partials[(size_t)row * PH_PART + tid] = (float)sum;
    }
}

// One thread per item: its channels' partials in fp64, channel by channel, then the constant factors of the chain rule.
__global__ void phaser_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ ctl, float* __restrict__ gctl, int B, int C,
                                       const PhCfg g) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s[PH_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const float* q = partials + ((size_t)b * C + c) * PH_PART;
#pragma unroll
        for (int k = 0; k < PH_PART; ++k) s[k] += (double)q[k];
    }
    const double ln2 = 0.6931471805599453, tau = 6.283185307179586, depth = (double)ctl[(size_t)b * 5 + 2];
    float* o = gctl + (size_t)b * 5;
    o[0] = (float)(tau * ln2 * depth / g.sr * s[0]);
    o[1] = (float)s[1];
    o[2] = (float)(ln2 * s[2]);
    o[3] = (float)(tau * ln2 * depth * s[3]);
    const float mix = ctl[(size_t)b * 5 + 4];
    o[4] = mix != mix ? mix : (float)s[4];                               // no term of it holds mix: a NaN mix makes the whole item NaN all the same
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline bool ph_k_ok(int K) { return K >= 1 && K <= PH_KMAX; }
inline long ph_ntile(long N) { return (N + PH_TILE - 1) / PH_TILE; }
inline size_t ph_lds_bytes(int K) { return (size_t)(K + 4) * PH_TILE * sizeof(float); }

// The backward kernel's rows are more LDS than a kernel gets unasked (64 KiB): asked for once per device - by dasp_phaser_prepare() when
// the library is loaded, so that no call has to (a call may be under stream capture) - and by the first call on any other device.
int ph_prepare() {
    static std::atomic<bool> asked[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (dev >= 0 && dev < 64 && asked[dev].load(std::memory_order_acquire)) return DASP_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(phaser_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)ph_lds_bytes(PH_KMAX));
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < 64) asked[dev].store(true, std::memory_order_release);
    return DASP_OK;
}

int ph_args(const float* x, const float* ctl, int B, int C, long N, int K, double sample_rate, double stereo_spread) {
    if (!x || !ctl || B <= 0 || C <= 0 || N <= 0 || K < 1 || !(sample_rate > 0.0) || !(sample_rate - sample_rate == 0.0) ||
        !(stereo_spread - stereo_spread == 0.0))
        return DASP_ERR_ARG;
    if (!ph_k_ok(K) || (long)B * C > 0x7fffffffL || ph_ntile(N) > 0x7fffffffL / PH_KMAX) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
inline PhCfg ph_cfg(double sample_rate, double stereo_spread) {
    return PhCfg{sample_rate, stereo_spread, 3.141592653589793 / sample_rate, (float)(sample_rate / 4096.0), (float)(0.49 * sample_rate)};
}
}  // namespace

extern "C" {

int dasp_phaser_max_stages(void) { return PH_KMAX; }
int dasp_phaser_tile(int stages) { return stages < 1 ? DASP_ERR_ARG : ph_k_ok(stages) ? PH_TILE : DASP_ERR_UNSUPPORTED; }
long dasp_phaser_state_floats(long rows, long N, int stages) {
    if (rows <= 0 || N <= 0 || stages < 1) return DASP_ERR_ARG;
    return ph_k_ok(stages) ? rows * ph_ntile(N) * stages : DASP_ERR_UNSUPPORTED;
}
long dasp_phaser_partial_floats(long rows) { return rows <= 0 ? DASP_ERR_ARG : rows * PH_PART; }
int dasp_phaser_prepare(void) { return ph_prepare(); }

int dasp_phaser_forward(const float* x, const float* ctl, float* y, float* states, int B, int C, long N, int stages, double sample_rate,
                        double stereo_spread, void* stream) {
    if (!y) return DASP_ERR_ARG;
    const int s = ph_args(x, ctl, B, C, N, stages, sample_rate, stereo_spread);
    if (s != DASP_OK) return s;
    const PhCfg g = ph_cfg(sample_rate, stereo_spread);
    const dim3 grid((unsigned)((long)B * C)), block(PH_THREADS);
    const int nt = (int)ph_ntile(N);
    if (states) hipLaunchKernelGGL(phaser_forward_kernel<true>, grid, block, 0, (hipStream_t)stream, x, ctl, y, states, N, nt, C, stages, g);
    else hipLaunchKernelGGL(phaser_forward_kernel<false>, grid, block, 0, (hipStream_t)stream, x, ctl, y, states, N, nt, C, stages, g);
    return launch_status();
}

int dasp_phaser_backward(const float* x, const float* ctl, const float* states, const float* gy, float* gx, float* gctl, float* partials, int B,
                         int C, long N, int stages, double sample_rate, double stereo_spread, void* stream) {
    if (!states || !gy || !gctl || !partials) return DASP_ERR_ARG;
    int s = ph_args(x, ctl, B, C, N, stages, sample_rate, stereo_spread);
    if (s != DASP_OK) return s;
    if ((s = ph_prepare()) != DASP_OK) return s;
    const PhCfg g = ph_cfg(sample_rate, stereo_spread);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(phaser_backward_kernel, dim3((unsigned)((long)B * C)), dim3(PH_THREADS), ph_lds_bytes(stages), st, x, ctl, states, gy, gx,
                       partials, N, (int)ph_ntile(N), C, stages, g);
    if ((s = launch_status()) != DASP_OK) return s;
    hipLaunchKernelGGL(phaser_finalize_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, st, (const float*)partials, ctl, gctl, B, C, g);
    return launch_status();
}

}  // extern "C"
