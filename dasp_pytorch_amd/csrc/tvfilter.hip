// time_varying_filter: Simper's trapezoidal state-variable filter (the published Cytomic form) whose cutoff and resonance follow control
// curves - the first recurrence of the library that couples two states, so that its scan composes 2 x 2 matrices instead of scalars.
//
//   frame points, float64 then rounded once:  G_j = tan(pi clamp(cutoff_hz[b,j], sr/4096, 0.49 sr) / sr),  K_j = 1 / clamp(q[b,j], 0.1, 100)
//   per sample, float32:  j = n / hop,  t = (n mod hop) / hop,  g = G_j + t (G_{j+1} - G_j),  k = K_j + t (K_{j+1} - K_j)
//     a1 = 1 / (1 + g (g + k)),  a2 = g a1,  a3 = g a2
//     v3 = x[n] - ic2,  v1 = a1 ic1 + a2 v3,  v2 = ic2 + a2 ic1 + a3 v3,  ic1 <- 2 v1 - ic1,  ic2 <- 2 v2 - ic2      (both zero before sample 0)
//     w = v2 (lowpass) | k v1 (bandpass) | x - k v1 - v2 (highpass) | x - k v1 (notch);   y[n] = (1 - mix) x[n] + mix w
// The curves are (B, F), F = ceil(N / hop) + 1, shared by an item's channels; hop is a power of two from 8 to 2048. The clamps are
// comparisons, which a NaN passes: a NaN frame value j makes its item NaN from sample (j - 1) hop on and nothing before it.
//
// With z = (ic1, ic2) a sample is the affine map z <- A[n] z + b[n] x[n], and maps compose: (A2, c2) after (A1, c1) = (A2 A1, A2 c1 + c2),
// six floats. ONE WORKGROUP OWNS ONE (b, c) ROW and walks it in tiles of 2048 samples; thread tid takes the 8 consecutive samples from
// 8 tid on, which lie inside one frame interval (hop >= 8), and a tile holds whole intervals (hop <= 2048). Per tile:
//   0  the tile's 2048 / hop + 1 frame points, one per thread, into LDS (tan in float64: N / hop times per row, not N times);
//   1  the thread's run from the two unit states and from zero state with its x: the run's map;
//   2  the scan of the maps over the lanes of a wave on DPP (row_shr 1, 2, 4, 8, row_bcast 15, 31) and over the four waves through LDS;
//   3  the run again from the state that comes in, in the form above - what is written is the recurrence itself, not a fixed-up sum.
// Two floats are carried from tile to tile; with `states` they are also saved, z before every tile: all the backward pass needs beyond
// x and the curves. x comes in and y goes out through LDS, a lane per consecutive sample on the global side (row stride 9 words on the
// LDS side); x is loaded one tile ahead. Forward traffic: 8 B per sample.
//
// Backward, the same walk from the last tile. Phase 1 is steps 0 - 2 from the saved state: z before every run, to LDS. Phase 2 runs in
// reverse time - thread r takes the run of thread 255 - r, last sample first, so that the same scan serves. It rebuilds z before each of
// its samples, then with gw = mix gy and mu[n] the gradient of z[n-1]:
//   q1 = 2 lam1 + gw dw/dv1,  q2 = 2 lam2 + gw dw/dv2,  gv3 = a2 q1 + a3 q2               (lam[n] = mu[n+1]; zero after the row)
//   mu[n] = (a1 q1 + a2 q2 - lam1,  q2 - lam2 - gv3)          = A[n]^T lam[n] + p[n] gw[n]: the forward scan with transposed matrices
//   gx[n] = (1 - mix) gy[n] + gv3 + gw dw/dx;   gmix = sum gy (w - x), w - x in a form that does not cancel where the filter passes x
//   ga1 = q1 ic1,  ga2 = q1 v3 + q2 ic1,  ga3 = q2 v3,  gk = gw dw/dk, chained through a1, a2, a3 to gg[n] and gk[n]
// A frame point collects (1 - t) gg over its own interval and t gg over the one before it. The sums are float32 per thread and tile and
// float64 from there on, in a fixed order: an xor butterfly over the lanes of an interval inside a wave, then the interval's waves, the
// interval before a frame point first. A frame point on a tile boundary takes the earlier tile's half, then the later tile's, which
// the walk carried along. A finalize kernel adds an item's channels in float64 and applies dG/dcutoff and dK/dq in float64, exactly
// zero where the frame value was clamped. No atomics anywhere: every result is bit-identical run to run and for an item alone or in a
// batch. Backward traffic: 12 B per sample. LDS: forward 20 KiB, backward 31 KiB.
#include "tv_scan.hpp"      // the tile geometry, tv_step, the maps and their scan, the interval sum: shared with tveq.hip

namespace dasp {

// wk = pi / sr; flo, fhi: the clamp of the cutoff; m1, m2, mx: w = m1 k v1 + m2 v2 + mx x;
// d2, dl, dx: w - x = m1 k v1 + d2 v2 + dl (a2 ic1 - a1 (1 + g k) v3) + dx x, the form without the cancellation of a pass band (tv_cfg)
struct TvCfg { double wk, flo, fhi; float m1, m2, mx, d2, dl, dx, inv_hop; int hop, lg; };

// The frame points j0 .. j0 + nfp - 1 of a tile; those past the curves (only runs past the row read them) are zero.
__device__ __forceinline__ void tv_frames(float* Gs, float* Ks, const float* __restrict__ cut, const float* __restrict__ q, long j0, int nfp, long F,
                                          const TvCfg& g, int tid) {
    for (int i = tid; i < nfp; i += TV_THREADS) {
        const long j = j0 + i;
        float G = 0.f, K = 0.f;
        if (j < F) {
            G = (float)tan(g.wk * tv_clamp((double)cut[j], g.flo, g.fhi));
            K = (float)(1.0 / tv_clamp((double)q[j], 0.1, 100.0));
        }
        Gs[i] = G;
        Ks[i] = K;
    }
}

// The coefficients of a thread's 8 samples: i0 its first sample in the tile.
__device__ __forceinline__ void tv_coef(TvRun& c, const float* Gs, const float* Ks, int i0, const TvCfg& g) {
    const int ii = i0 >> g.lg, off = i0 & (g.hop - 1);
    const float G0 = Gs[ii], dG = Gs[ii + 1] - G0, K0 = Ks[ii], dK = Ks[ii + 1] - K0;
#pragma unroll
    for (int j = 0; j < TV_SPT; ++j) {
        c.t[j] = (float)(off + j) * g.inv_hop;      // exact: hop is a power of two
        c.g[j] = __builtin_fmaf(c.t[j], dG, G0);
        c.k[j] = __builtin_fmaf(c.t[j], dK, K0);
        c.a1[j] = 1.f / __builtin_fmaf(c.g[j], c.g[j] + c.k[j], 1.f);
        c.a2[j] = c.g[j] * c.a1[j];
        c.a3[j] = c.g[j] * c.a2[j];
    }
}

// One sample of the adjoint: lam = (l1, l2) the gradient of the state after the sample, mu that of the state before it.
__device__ __forceinline__ void tv_adj(float l1, float l2, float gw, float k, float a1, float a2, float a3, const TvCfg& g, float& q1, float& q2, float& gv3,
                                       float& mu1, float& mu2) {
    q1 = __builtin_fmaf(gw, g.m1 * k, 2.f * l1);
    q2 = __builtin_fmaf(gw, g.m2, 2.f * l2);
    gv3 = __builtin_fmaf(q1, a2, q2 * a3);
    mu1 = __builtin_fmaf(q1, a1, __builtin_fmaf(q2, a2, -l1));
    mu2 = (q2 - l2) - gv3;
}

template <bool SAVE>
__global__ void __launch_bounds__(TV_THREADS)
tvfilter_forward_kernel(const float* __restrict__ x, const float* __restrict__ cut, const float* __restrict__ q, const float* __restrict__ mixv,
                        float* __restrict__ y, float* __restrict__ states, long N, int ntile, int C, long F, const TvCfg g) {
    __shared__ float xs[TV_STAGE], ys[TV_STAGE];
    __shared__ float Gs[TV_FP], Ks[TV_FP];
    __shared__ float wt[6 * TV_NW];
    __shared__ float carry[2][2];
    const int row = blockIdx.x, tid = threadIdx.x, b = row / C;
    const float mix = mixv[b], dry = 1.f - mix;
    const float* xr = x + (size_t)row * N;
    const float* cr = cut + (size_t)b * F;
    const float* qr = q + (size_t)b * F;
    float* yr = y + (size_t)row * N;
    float* sr = SAVE ? states + (size_t)row * ntile * 2 : nullptr;
    const int nint = TV_TILE >> g.lg;

    if (tid < 2) {
        carry[0][tid] = 0.f;
        if (SAVE) sr[tid] = 0.f;                         // the state before the row
    }
    float xn[TV_SPT];
    stage_load<TV_SPT, TV_THREADS>(xn, xr, 0, N, tid);
    int par = 0;
    for (int ti = 0; ti < ntile; ++ti) {
        const long t0 = (long)ti * TV_TILE;
        stage_put<TV_SPT, TV_THREADS>(xs, xn, tid);
        tv_frames(Gs, Ks, cr, qr, t0 >> g.lg, nint + 1, F, g, tid);
        stage_load<TV_SPT, TV_THREADS>(xn, xr, t0 + TV_TILE, N, tid);
        lds_barrier();

        const int i0 = tid * TV_SPT;
        float xv[TV_SPT];
        TvRun c;
        tv_coef(c, Gs, Ks, i0, g);
#pragma unroll
        for (int j = 0; j < TV_SPT; ++j) xv[j] = xs[stage_word<TV_SPT>(i0 + j)];
        float z1, z2;
        tv_scan(tv_run_map(xv, c), carry[par][0], carry[par][1], wt, z1, z2);
#pragma unroll
        for (int j = 0; j < TV_SPT; ++j) {
            float v1, v2;
            tv_step(z1, z2, xv[j], c.a1[j], c.a2[j], c.a3[j], v1, v2);
            const float w = __builtin_fmaf(g.m1 * c.k[j], v1, __builtin_fmaf(g.m2, v2, g.mx * xv[j]));
            ys[stage_word<TV_SPT>(i0 + j)] = __builtin_fmaf(mix, w, dry * xv[j]);
        }
        if (tid == TV_THREADS - 1) {
            carry[par ^ 1][0] = z1;
            carry[par ^ 1][1] = z2;
            if (SAVE && ti + 1 < ntile) { sr[(size_t)(ti + 1) * 2] = z1; sr[(size_t)(ti + 1) * 2 + 1] = z2; }
        }
        lds_barrier();
        const int Tc = (int)min((long)TV_TILE, N - t0);
        for (int i = tid; i < Tc; i += TV_THREADS) st_stream(yr + t0 + i, ys[stage_word<TV_SPT>(i)]);
        par ^= 1;
    }
}

// partials: per row 2 F + 1 floats - the row's sums for G_j, for K_j, for mix.
__global__ void __launch_bounds__(TV_THREADS)
tvfilter_backward_kernel(const float* __restrict__ x, const float* __restrict__ cut, const float* __restrict__ q, const float* __restrict__ mixv,
                         const float* __restrict__ states, const float* __restrict__ gy, float* __restrict__ gx, float* __restrict__ partials, long N,
                         int ntile, int C, long F, const TvCfg g) {
    __shared__ float s1[TV_STAGE], s2[TV_STAGE];                          // x; gy, then gx
    __shared__ float Gs[TV_FP], Ks[TV_FP];
    __shared__ float wt[6 * TV_NW];
    __shared__ float zin[2 * TV_THREADS];
    __shared__ float cst[2], clam[2][2];
    __shared__ double red[TV_THREADS][4];                                 // per group of lanes: own interval's G, next frame point's G, the same for K
    __shared__ double edge[2][2];                                         // what the later tile found for the frame point on the boundary
    __shared__ double rmix[TV_NW];
    const int row = blockIdx.x, tid = threadIdx.x, b = row / C;
    const float mix = mixv[b], dry = 1.f - mix;
    const float* xr = x + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;
    const float* cr = cut + (size_t)b * F;
    const float* qr = q + (size_t)b * F;
    const float* sr = states + (size_t)row * ntile * 2;
    float* gxr = gx ? gx + (size_t)row * N : nullptr;
    float* pr = partials + (size_t)row * (2 * (size_t)F + 1);
    const int nint = TV_TILE >> g.lg;
    const int R = g.hop / TV_SPT, W = R < 64 ? R : 64, S = R / W;         // runs of an interval; lanes of a group; groups of an interval

    if (tid < 2) { clam[0][tid] = 0.f; edge[0][tid] = 0.0; }
    float xn[TV_SPT], gn[TV_SPT];
    stage_load<TV_SPT, TV_THREADS>(xn, xr, (long)(ntile - 1) * TV_TILE, N, tid);
    stage_load<TV_SPT, TV_THREADS>(gn, gr, (long)(ntile - 1) * TV_TILE, N, tid);
    double s_mix = 0.0;
    int par = 0;
    for (int ti = ntile - 1; ti >= 0; --ti) {
        const long t0 = (long)ti * TV_TILE, j0 = t0 >> g.lg;
        stage_put<TV_SPT, TV_THREADS>(s1, xn, tid);
        stage_put<TV_SPT, TV_THREADS>(s2, gn, tid);
        tv_frames(Gs, Ks, cr, qr, j0, nint + 1, F, g, tid);
        if (tid < 2) cst[tid] = ti ? sr[(size_t)ti * 2 + tid] : 0.f;
        stage_load<TV_SPT, TV_THREADS>(xn, xr, t0 - TV_TILE, N, tid);
        stage_load<TV_SPT, TV_THREADS>(gn, gr, t0 - TV_TILE, N, tid);
        lds_barrier();

        // ---- phase 1, forward time: the state before the run of every thread
        {
            const int i0 = tid * TV_SPT;
            float xv[TV_SPT], z1, z2;
            TvRun c;
            tv_coef(c, Gs, Ks, i0, g);
#pragma unroll
            for (int j = 0; j < TV_SPT; ++j) xv[j] = s1[stage_word<TV_SPT>(i0 + j)];
            tv_scan(tv_run_map(xv, c), cst[0], cst[1], wt, z1, z2);
            zin[2 * tid] = z1;
            zin[2 * tid + 1] = z2;
        }
        lds_barrier();

        // ---- phase 2, reverse time: thread tid has the run of thread f = 255 - tid; m = 0 is its last sample, j = 7 - m
        float p_gl = 0.f, p_gr = 0.f, p_kl = 0.f, p_kr = 0.f, t_mix = 0.f;
        const int f = TV_THREADS - 1 - tid;
        {
            const int i0 = f * TV_SPT;
            float xv[TV_SPT], gv[TV_SPT], zp1[TV_SPT], zp2[TV_SPT], vv1[TV_SPT];
            TvRun c;
            tv_coef(c, Gs, Ks, i0, g);
            float z1 = zin[2 * f], z2 = zin[2 * f + 1];
#pragma unroll
            for (int j = 0; j < TV_SPT; ++j) {
                xv[j] = s1[stage_word<TV_SPT>(i0 + j)];
                gv[j] = s2[stage_word<TV_SPT>(i0 + j)];
                zp1[j] = z1;
                zp2[j] = z2;
                float v2;
                tv_step(z1, z2, xv[j], c.a1[j], c.a2[j], c.a3[j], vv1[j], v2);
                const float lp = __builtin_fmaf(c.a2[j], zp1[j], -(c.a1[j] * __builtin_fmaf(c.g[j], c.k[j], 1.f)) * (xv[j] - zp2[j]));
                const float d = __builtin_fmaf(g.m1 * c.k[j], vv1[j], __builtin_fmaf(g.d2, v2, __builtin_fmaf(g.dl, lp, g.dx * xv[j])));
                t_mix = __builtin_fmaf(gv[j], t0 + i0 + j < N ? d : 0.f, t_mix);
            }
            // the run's map in reverse time: from the two unit gradients without gw, and from zero with the run's gw
            float e1 = 1.f, e2 = 0.f, f1 = 0.f, f2 = 1.f, l1 = 0.f, l2 = 0.f;
#pragma unroll
            for (int m = 0; m < TV_SPT; ++m) {
                const int j = TV_SPT - 1 - m;
                float q1, q2, gv3, n1, n2;
                tv_adj(e1, e2, 0.f, c.k[j], c.a1[j], c.a2[j], c.a3[j], g, q1, q2, gv3, n1, n2); e1 = n1; e2 = n2;
                tv_adj(f1, f2, 0.f, c.k[j], c.a1[j], c.a2[j], c.a3[j], g, q1, q2, gv3, n1, n2); f1 = n1; f2 = n2;
                tv_adj(l1, l2, mix * gv[j], c.k[j], c.a1[j], c.a2[j], c.a3[j], g, q1, q2, gv3, n1, n2); l1 = n1; l2 = n2;
            }
            tv_scan(TvMap{e1, f1, e2, f2, l1, l2}, clam[par][0], clam[par][1], wt, l1, l2);
#pragma unroll
            for (int m = 0; m < TV_SPT; ++m) {
                const int j = TV_SPT - 1 - m;
                const float gw = mix * gv[j];
                float q1, q2, gv3, n1, n2;
                tv_adj(l1, l2, gw, c.k[j], c.a1[j], c.a2[j], c.a3[j], g, q1, q2, gv3, n1, n2);
                s2[stage_word<TV_SPT>(i0 + j)] = __builtin_fmaf(dry, gv[j], __builtin_fmaf(gw, g.mx, gv3));
                const float v3 = xv[j] - zp2[j];
                const float ga3 = q2 * v3;
                const float ga2 = __builtin_fmaf(c.g[j], ga3, __builtin_fmaf(q1, v3, q2 * zp1[j]));
                const float ga1 = __builtin_fmaf(c.g[j], ga2, q1 * zp1[j]);
                const float gd = -(c.a1[j] * c.a1[j]) * ga1;                             // 1 / a1 = 1 + g (g + k)
                float gg = __builtin_fmaf(c.a2[j], ga3, __builtin_fmaf(c.a1[j], ga2, (c.g[j] + c.g[j] + c.k[j]) * gd));
                float gk = __builtin_fmaf(c.g[j], gd, gw * g.m1 * vv1[j]);
                if (!(t0 + i0 + j < N)) gg = gk = 0.f;
                const float t = c.t[j], u = 1.f - t;
                p_gl = __builtin_fmaf(u, gg, p_gl);
                p_gr = __builtin_fmaf(t, gg, p_gr);
                p_kl = __builtin_fmaf(u, gk, p_kl);
                p_kr = __builtin_fmaf(t, gk, p_kr);
                l1 = n1;
                l2 = n2;
            }
            if (tid == TV_THREADS - 1) { clam[par ^ 1][0] = l1; clam[par ^ 1][1] = l2; }
        }
        s_mix += (double)t_mix;
        // the runs of an interval: the lanes of a group by an xor butterfly, every lane of it ending with the same bits
        {
            double d[4] = {(double)p_gl, (double)p_gr, (double)p_kl, (double)p_kr};
            tv_group_sum(d, W);
            if ((tid & (W - 1)) == 0) {
                double* o = red[f / W];
                o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3];
            }
        }
        lds_barrier();
        // frame point i of the tile: the interval before it, then its own, then - on the tile's end - what the later tile carried
        for (int i = tid; i <= nint; i += TV_THREADS) {
            double sg = 0.0, sk = 0.0;
            if (i > 0)
                for (int s = 0; s < S; ++s) { sg += red[(i - 1) * S + s][1]; sk += red[(i - 1) * S + s][3]; }
            if (i < nint)
                for (int s = 0; s < S; ++s) { sg += red[i * S + s][0]; sk += red[i * S + s][2]; }
            if (i == nint) { sg += edge[par][0]; sk += edge[par][1]; }
            if (i == 0 && ti > 0) {
                edge[par ^ 1][0] = sg;
                edge[par ^ 1][1] = sk;
            } else if (j0 + i < F) {
                pr[j0 + i] = (float)sg;
                pr[F + j0 + i] = (float)sk;
            }
        }
        if (gxr) {
            const int Tc = (int)min((long)TV_TILE, N - t0);
            for (int i = tid; i < Tc; i += TV_THREADS) st_stream(gxr + t0 + i, s2[stage_word<TV_SPT>(i)]);
        }
        lds_barrier();                                // red, s1, s2 and zin are written again by the next tile
        par ^= 1;
    }
    s_mix = wave_sum(s_mix);
    if (lane_id() == 0) rmix[wave_id()] = s_mix;
    __syncthreads();
    if (tid == 0) {
        double sum = rmix[0];
#pragma unroll
        for (int u = 1; u < TV_NW; ++u) sum += rmix[u];
        pr[2 * (size_t)F] = (float)sum;
    }
}

// One thread per (item, frame point): its channels' sums in float64, channel by channel, then dG / dcutoff and dK / dq in float64 - exactly
// zero where the frame value was clamped. The thread of frame point 0 also adds the item's mix.
__global__ void tvfilter_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ cut, const float* __restrict__ q,
                                         const float* __restrict__ mixv, float* __restrict__ gcut, float* __restrict__ gq, float* __restrict__ gmix, int B, int C,
                                         long F, const TvCfg g) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)B * F) return;
    const long b = id / F, j = id - b * F;
    const size_t stride = 2 * (size_t)F + 1;
    double sg = 0.0, sk = 0.0, sm = 0.0;
    for (int c = 0; c < C; ++c) {
        const float* p = partials + ((size_t)b * C + c) * stride;
        sg += (double)p[j];
        sk += (double)p[F + j];
        if (j == 0) sm += (double)p[2 * (size_t)F];
    }
    const double cv = (double)cut[id], qv = (double)q[id];
    const double G = tan(g.wk * tv_clamp(cv, g.flo, g.fhi));
    gcut[id] = cv < g.flo || cv > g.fhi ? 0.f : (float)(sg * g.wk * (1.0 + G * G));
    gq[id] = qv < 0.1 || qv > 100.0 ? 0.f : (float)(-sk / (qv * qv));
    if (j == 0) {
        const float mix = mixv[b];
        gmix[b] = mix != mix ? mix : (float)sm;          // no term of it holds mix: a NaN mix makes the whole item NaN all the same
    }
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
int tv_args(const float* x, const float* cut, const float* q, const float* mix, int B, int C, long N, int hop, int mode, double sample_rate) {
    if (!x || !cut || !q || !mix || B <= 0 || C <= 0 || N <= 0 || hop <= 0 || mode < 0 || mode > 3 || !(sample_rate > 0.0) ||
        !(sample_rate - sample_rate == 0.0))
        return DASP_ERR_ARG;
    if (!tv_hop_ok(hop) || (long)B * C > 0x7fffffffL || tv_ntile(N) > 0x3fffffffL || (long)B > 0x7fffffffL * 64 / tv_frames_of(N, hop))
        return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
inline TvCfg tv_cfg(double sample_rate, int hop, int mode) {
    // lowpass, bandpass, highpass, notch. w - x: where w holds x it drops out (highpass, notch); the low-pass's v2 - x, which cancels where
    // the cutoff is high, is (1 - a3)(ic2 - x) + a2 ic1 with 1 - a3 = a1 (1 + g k)
    static const float M[4][6] = {{0.f, 1.f, 0.f, 0.f, 1.f, 0.f}, {1.f, 0.f, 0.f, 0.f, 0.f, -1.f}, {-1.f, -1.f, 1.f, -1.f, 0.f, 0.f}, {-1.f, 0.f, 1.f, 0.f, 0.f, 0.f}};
    int lg = 0;
    while ((1 << lg) < hop) ++lg;
    return TvCfg{3.141592653589793 / sample_rate, sample_rate / 4096.0, 0.49 * sample_rate, M[mode][0], M[mode][1], M[mode][2],
                 M[mode][3], M[mode][4], M[mode][5], 1.f / (float)hop, hop, lg};
}
}  // namespace

extern "C" {

int dasp_tvfilter_tile(void) { return TV_TILE; }
long dasp_tvfilter_frames(long N, int hop) {
    if (N <= 0 || hop <= 0) return DASP_ERR_ARG;
    return tv_hop_ok(hop) ? tv_frames_of(N, hop) : DASP_ERR_UNSUPPORTED;
}
long dasp_tvfilter_state_floats(long rows, long N) { return rows <= 0 || N <= 0 ? DASP_ERR_ARG : rows * tv_ntile(N) * 2; }
long dasp_tvfilter_scratch_floats(long rows, long N, int hop) {
    if (rows <= 0 || N <= 0 || hop <= 0) return DASP_ERR_ARG;
    return tv_hop_ok(hop) ? rows * (2 * tv_frames_of(N, hop) + 1) : DASP_ERR_UNSUPPORTED;
}

int dasp_tvfilter_forward(const float* x, const float* cutoff_hz, const float* q, const float* mix, float* y, float* states, int B, int C, long N,
                          int hop, int mode, double sample_rate, void* stream) {
    if (!y) return DASP_ERR_ARG;
    const int s = tv_args(x, cutoff_hz, q, mix, B, C, N, hop, mode, sample_rate);
    if (s != DASP_OK) return s;
    const TvCfg g = tv_cfg(sample_rate, hop, mode);
    const dim3 grid((unsigned)((long)B * C)), block(TV_THREADS);
    const int nt = (int)tv_ntile(N);
    const long F = tv_frames_of(N, hop);
    if (states) hipLaunchKernelGGL(tvfilter_forward_kernel<true>, grid, block, 0, (hipStream_t)stream, x, cutoff_hz, q, mix, y, states, N, nt, C, F, g);
    else hipLaunchKernelGGL(tvfilter_forward_kernel<false>, grid, block, 0, (hipStream_t)stream, x, cutoff_hz, q, mix, y, states, N, nt, C, F, g);
    return launch_status();
}

int dasp_tvfilter_backward(const float* x, const float* cutoff_hz, const float* q, const float* mix, const float* states, const float* gy, float* gx,
                           float* gcutoff, float* gq, float* gmix, float* scratch, int B, int C, long N, int hop, int mode, double sample_rate,
                           void* stream) {
    if (!states || !gy || !gcutoff || !gq || !gmix || !scratch) return DASP_ERR_ARG;
    int s = tv_args(x, cutoff_hz, q, mix, B, C, N, hop, mode, sample_rate);
    if (s != DASP_OK) return s;
    const TvCfg g = tv_cfg(sample_rate, hop, mode);
    const hipStream_t st = (hipStream_t)stream;
    const long F = tv_frames_of(N, hop);
    hipLaunchKernelGGL(tvfilter_backward_kernel, dim3((unsigned)((long)B * C)), dim3(TV_THREADS), 0, st, x, cutoff_hz, q, mix, states, gy, gx, scratch, N,
                       (int)tv_ntile(N), C, F, g);
    if ((s = launch_status()) != DASP_OK) return s;
    hipLaunchKernelGGL(tvfilter_finalize_kernel, dim3((unsigned)(((long)B * F + 127) / 128)), dim3(128), 0, st, (const float*)scratch, cutoff_hz, q, mix,
                       gcutoff, gq, gmix, B, C, F, g);
    return launch_status();
}

}  // extern "C"
