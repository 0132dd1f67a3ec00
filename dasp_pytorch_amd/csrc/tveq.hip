// time_varying_eq: a bell, low-shelf or high-shelf band of Simper's trapezoidal state-variable filter whose gain, cutoff and Q follow
// control curves - the recurrence and the walk of tvfilter.hip with a third curve, which enters the recurrence (k for the bell, g for the
// shelves) as well as the output map.
//
//   frame points, float64 then rounded once:  A_j = 10^(clamp(gain_db[b,j], -40, 40) / 40),  T_j = tan(pi clamp(cutoff_hz[b,j], sr/4096, 0.49 sr) / sr),
//     Qc = clamp(q[b,j], 0.1, 100);   bell: G_j = T_j, K_j = 1 / (Qc A_j)   lowshelf: G_j = T_j / sqrt A_j, K_j = 1 / Qc   highshelf: G_j = T_j sqrt A_j, K_j = 1 / Qc
//   per sample, float32:  j = n / hop,  t = (n mod hop) / hop,  g = G_j + t (G_{j+1} - G_j),  likewise k from K and A from A_j
//     a1, a2, a3, v1, v2 and the two states as in tvfilter.hip (tv_step)
//     y[n] = x + k (A^2 - 1) v1 (bell) | x + k (A - 1) v1 + (A^2 - 1) v2 (lowshelf) | A^2 x + k (1 - A) A v1 + (1 - A^2) v2 (highshelf)
// written below as y = cx x + c1 v1 + c2 v2 (tveq_out). A = 1 gives c1 = c2 = 0 and cx = 1 exactly: y = x and gx = gy bit for bit.
// The curves are (B, F), F = ceil(N / hop) + 1, shared by an item's channels; hop is a power of two from 8 to 2048. The clamps are
// comparisons, which a NaN passes: a NaN frame value j makes its item NaN from sample (j - 1) hop on and nothing before it.
//
// The walk is that of tvfilter.hip, on the pieces of tv_scan.hpp: one workgroup per (b, c) row, tiles of 2048 samples, 8 consecutive
// samples per thread, the scan of the runs' 2 x 2 maps on DPP and through LDS, x staged one tile ahead, two states per tile saved when
// a gradient is wanted. Forward traffic: 8 B per sample.
//
// Backward, the same walk from the last tile, in the two phases of tvfilter_backward_kernel. With lam[n] the gradient of the state after
// sample n and mu[n] that of the state before it:
//   q1 = 2 lam1 + gy c1,  q2 = 2 lam2 + gy c2,  gv3 = a2 q1 + a3 q2,  mu = (a1 q1 + a2 q2 - lam1,  q2 - lam2 - gv3),  gx[n] = cx gy[n] + gv3
//   ga1, ga2, ga3 chained to gg[n] and gk[n] as there;  gk[n] += gy dy/dk,  gA[n] = gy dy/dA:
//     dy/dk = (A^2 - 1) v1 | (A - 1) v1 | (1 - A) A v1;     dy/dA = 2 A k v1 | k v1 + 2 A v2 | 2 A (x - v2) + k (1 - 2 A) v1
// v1 and v2 are rebuilt from the state before the sample, not held. A frame point collects (1 - t) of its own interval and t of the one
// before it, for g, k and A, in the fixed order of tvfilter.hip: float32 per thread and tile, float64 from there on, the xor butterfly
// over an interval's lanes, then its waves, the earlier tile's half of a boundary point first. The finalize kernel adds an item's
// channels and chains (gG, gK, gA) to the three curves in float64 (tveq_finalize_kernel), exactly zero where a frame value was clamped.
// No atomics anywhere. Backward traffic: 12 B per sample. LDS: forward 21 KiB, backward 36 KiB.
#include "tv_scan.hpp"

namespace dasp {

// wk = pi / sr; flo, fhi: the clamp of the cutoff
struct TveqCfg { double wk, flo, fhi; float inv_hop; int hop, lg; };

constexpr double TVEQ_DB_MAX = 40.0, TVEQ_Q_LO = 0.1, TVEQ_Q_HI = 100.0;
enum { TVEQ_BELL = 0, TVEQ_LOWSHELF = 1, TVEQ_HIGHSHELF = 2 };

// A, T and the clamped Q of one frame point, and from them G and K; float64
struct TveqPoint { double A, T, Q, G, K; };
__device__ __forceinline__ TveqPoint tveq_point(double gain_db, double cutoff, double q, int mode, const TveqCfg& g) {
    TveqPoint p;
    p.A = pow(10.0, tv_clamp(gain_db, -TVEQ_DB_MAX, TVEQ_DB_MAX) / 40.0);
    p.T = tan(g.wk * tv_clamp(cutoff, g.flo, g.fhi));
    p.Q = tv_clamp(q, TVEQ_Q_LO, TVEQ_Q_HI);
    if (mode == TVEQ_BELL) {
        p.G = p.T;
        p.K = 1.0 / (p.Q * p.A);
    } else {
        const double r = sqrt(p.A);
        p.G = mode == TVEQ_LOWSHELF ? p.T / r : p.T * r;
        p.K = 1.0 / p.Q;
    }
    return p;
}

// The frame points j0 .. j0 + nfp - 1 of a tile; those past the curves (only runs past the row read them) are zero.
template <int MODE>
__device__ __forceinline__ void tveq_frames(float* Gs, float* Ks, float* As, const float* __restrict__ gain, const float* __restrict__ cut,
                                            const float* __restrict__ q, long j0, int nfp, long F, const TveqCfg& g, int tid) {
    for (int i = tid; i < nfp; i += TV_THREADS) {
        const long j = j0 + i;
        float G = 0.f, K = 0.f, A = 0.f;
        if (j < F) {
            const TveqPoint p = tveq_point((double)gain[j], (double)cut[j], (double)q[j], MODE, g);
            G = (float)p.G;
            K = (float)p.K;
            A = (float)p.A;
        }
        Gs[i] = G;
        Ks[i] = K;
        As[i] = A;
    }
}

// The coefficients of a thread's 8 samples: i0 its first sample in the tile.
struct TveqRun { TvRun r; float A[TV_SPT]; };
__device__ __forceinline__ void tveq_coef(TveqRun& c, const float* Gs, const float* Ks, const float* As, int i0, const TveqCfg& g) {
    const int ii = i0 >> g.lg, off = i0 & (g.hop - 1);
    const float G0 = Gs[ii], dG = Gs[ii + 1] - G0, K0 = Ks[ii], dK = Ks[ii + 1] - K0, A0 = As[ii], dA = As[ii + 1] - A0;
#pragma unroll
    for (int j = 0; j < TV_SPT; ++j) {
        c.r.t[j] = (float)(off + j) * g.inv_hop;    // exact: hop is a power of two
        c.r.g[j] = __builtin_fmaf(c.r.t[j], dG, G0);
        c.r.k[j] = __builtin_fmaf(c.r.t[j], dK, K0);
        c.A[j] = __builtin_fmaf(c.r.t[j], dA, A0);
        c.r.a1[j] = 1.f / __builtin_fmaf(c.r.g[j], c.r.g[j] + c.r.k[j], 1.f);
        c.r.a2[j] = c.r.g[j] * c.r.a1[j];
        c.r.a3[j] = c.r.g[j] * c.r.a2[j];
    }
}

// The output map of a sample: y = cx x + c1 v1 + c2 v2. The bell has no c2 and only the high shelf a cx other than 1.
template <int MODE> __device__ __forceinline__ void tveq_out(float k, float A, float& c1, float& c2, float& cx) {
    const float e = __builtin_fmaf(A, A, -1.f);
    if (MODE == TVEQ_BELL) {
        c1 = k * e; c2 = 0.f; cx = 1.f;
    } else if (MODE == TVEQ_LOWSHELF) {
        c1 = k * (A - 1.f); c2 = e; cx = 1.f;
    } else {
        c1 = k * ((1.f - A) * A); c2 = -e; cx = A * A;
    }
}
template <int MODE> __device__ __forceinline__ float tveq_y(float x, float v1, float v2, float k, float A) {
    float c1, c2, cx;
    tveq_out<MODE>(k, A, c1, c2, cx);
    if (MODE == TVEQ_BELL) return __builtin_fmaf(c1, v1, x);
    if (MODE == TVEQ_LOWSHELF) return __builtin_fmaf(c1, v1, __builtin_fmaf(c2, v2, x));
    return __builtin_fmaf(cx, x, __builtin_fmaf(c1, v1, c2 * v2));
}

// One sample of the adjoint: lam = (l1, l2) the gradient of the state after the sample, mu that of the state before it; g1 = gy c1, g2 = gy c2.
__device__ __forceinline__ void tveq_adj(float l1, float l2, float g1, float g2, float a1, float a2, float a3, float& q1, float& q2, float& gv3, float& mu1,
                                         float& mu2) {
    q1 = __builtin_fmaf(2.f, l1, g1);
    q2 = __builtin_fmaf(2.f, l2, g2);
    gv3 = __builtin_fmaf(q1, a2, q2 * a3);
    mu1 = __builtin_fmaf(q1, a1, __builtin_fmaf(q2, a2, -l1));
    mu2 = (q2 - l2) - gv3;
}

template <int MODE, bool SAVE>
__global__ void __launch_bounds__(TV_THREADS)
tveq_forward_kernel(const float* __restrict__ x, const float* __restrict__ gain, const float* __restrict__ cut, const float* __restrict__ q,
                    float* __restrict__ y, float* __restrict__ states, long N, int ntile, int C, long F, const TveqCfg g) {
    __shared__ float xs[TV_STAGE], ys[TV_STAGE];
    __shared__ float Gs[TV_FP], Ks[TV_FP], As[TV_FP];
    __shared__ float wt[6 * TV_NW];
    __shared__ float carry[2][2];
    const int row = blockIdx.x, tid = threadIdx.x, b = row / C;
    const float* xr = x + (size_t)row * N;
    const float* ar = gain + (size_t)b * F;
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
        tveq_frames<MODE>(Gs, Ks, As, ar, cr, qr, t0 >> g.lg, nint + 1, F, g, tid);
        stage_load<TV_SPT, TV_THREADS>(xn, xr, t0 + TV_TILE, N, tid);
        lds_barrier();

        const int i0 = tid * TV_SPT;
        float xv[TV_SPT];
        TveqRun c;
        tveq_coef(c, Gs, Ks, As, i0, g);
#pragma unroll
        for (int j = 0; j < TV_SPT; ++j) xv[j] = xs[stage_word<TV_SPT>(i0 + j)];
        float z1, z2;
        tv_scan(tv_run_map(xv, c.r), carry[par][0], carry[par][1], wt, z1, z2);
#pragma unroll
        for (int j = 0; j < TV_SPT; ++j) {
            float v1, v2;
            tv_step(z1, z2, xv[j], c.r.a1[j], c.r.a2[j], c.r.a3[j], v1, v2);
            ys[stage_word<TV_SPT>(i0 + j)] = tveq_y<MODE>(xv[j], v1, v2, c.r.k[j], c.A[j]);
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

// partials: per row 3 F floats - the row's sums for G_j, for K_j, for A_j.
template <int MODE>
__global__ void __launch_bounds__(TV_THREADS)
tveq_backward_kernel(const float* __restrict__ x, const float* __restrict__ gain, const float* __restrict__ cut, const float* __restrict__ q,
                     const float* __restrict__ states, const float* __restrict__ gy, float* __restrict__ gx, float* __restrict__ partials, long N, int ntile,
                     int C, long F, const TveqCfg g) {
    __shared__ float s1[TV_STAGE], s2[TV_STAGE];                          // x; gy, then gx
    __shared__ float Gs[TV_FP], Ks[TV_FP], As[TV_FP];
    __shared__ float wt[6 * TV_NW];
    __shared__ float zin[2 * TV_THREADS];
    __shared__ float cst[2], clam[2][2];
    __shared__ double red[TV_THREADS][6];                                 // per group of lanes: own interval's, next frame point's - for G, K, A
    __shared__ double edge[2][3];                                         // what the later tile found for the frame point on the boundary
    const int row = blockIdx.x, tid = threadIdx.x, b = row / C;
    const float* xr = x + (size_t)row * N;
    const float* gr = gy + (size_t)row * N;
    const float* ar = gain + (size_t)b * F;
    const float* cr = cut + (size_t)b * F;
    const float* qr = q + (size_t)b * F;
    const float* sr = states + (size_t)row * ntile * 2;
    float* gxr = gx ? gx + (size_t)row * N : nullptr;
    float* pr = partials + (size_t)row * 3 * (size_t)F;
    const int nint = TV_TILE >> g.lg;
    const int R = g.hop / TV_SPT, W = R < 64 ? R : 64, S = R / W;         // runs of an interval; lanes of a group; groups of an interval

    if (tid < 2) clam[0][tid] = 0.f;
    if (tid < 3) edge[0][tid] = 0.0;
    float xn[TV_SPT], gn[TV_SPT];
    stage_load<TV_SPT, TV_THREADS>(xn, xr, (long)(ntile - 1) * TV_TILE, N, tid);
    stage_load<TV_SPT, TV_THREADS>(gn, gr, (long)(ntile - 1) * TV_TILE, N, tid);
    int par = 0;
    for (int ti = ntile - 1; ti >= 0; --ti) {
        const long t0 = (long)ti * TV_TILE, j0 = t0 >> g.lg;
        stage_put<TV_SPT, TV_THREADS>(s1, xn, tid);
        stage_put<TV_SPT, TV_THREADS>(s2, gn, tid);
        tveq_frames<MODE>(Gs, Ks, As, ar, cr, qr, j0, nint + 1, F, g, tid);
        if (tid < 2) cst[tid] = ti ? sr[(size_t)ti * 2 + tid] : 0.f;
        stage_load<TV_SPT, TV_THREADS>(xn, xr, t0 - TV_TILE, N, tid);
        stage_load<TV_SPT, TV_THREADS>(gn, gr, t0 - TV_TILE, N, tid);
        lds_barrier();

        // ---- phase 1, forward time: the state before the run of every thread
        {
            const int i0 = tid * TV_SPT;
            float xv[TV_SPT], z1, z2;
            TveqRun c;
            tveq_coef(c, Gs, Ks, As, i0, g);
#pragma unroll
            for (int j = 0; j < TV_SPT; ++j) xv[j] = s1[stage_word<TV_SPT>(i0 + j)];
            tv_scan(tv_run_map(xv, c.r), cst[0], cst[1], wt, z1, z2);
            zin[2 * tid] = z1;
            zin[2 * tid + 1] = z2;
        }
        lds_barrier();

        // ---- phase 2, reverse time: thread tid has the run of thread f = 255 - tid; m = 0 is its last sample, j = 7 - m
        float p_gl = 0.f, p_gr = 0.f, p_kl = 0.f, p_kr = 0.f, p_al = 0.f, p_ar = 0.f;
        const int f = TV_THREADS - 1 - tid;
        {
            const int i0 = f * TV_SPT;
            float xv[TV_SPT], gv[TV_SPT], zp1[TV_SPT], zp2[TV_SPT];
            TveqRun c;
            tveq_coef(c, Gs, Ks, As, i0, g);
            float z1 = zin[2 * f], z2 = zin[2 * f + 1];
#pragma unroll
            for (int j = 0; j < TV_SPT; ++j) {
                xv[j] = s1[stage_word<TV_SPT>(i0 + j)];
                gv[j] = s2[stage_word<TV_SPT>(i0 + j)];
                zp1[j] = z1;
                zp2[j] = z2;
                float v1, v2;
                tv_step(z1, z2, xv[j], c.r.a1[j], c.r.a2[j], c.r.a3[j], v1, v2);
            }
            // the run's map in reverse time: from the two unit gradients without gy, and from zero with the run's gy
            float e1 = 1.f, e2 = 0.f, f1 = 0.f, f2 = 1.f, l1 = 0.f, l2 = 0.f;
#pragma unroll
            for (int m = 0; m < TV_SPT; ++m) {
                const int j = TV_SPT - 1 - m;
                float c1, c2, cx, q1, q2, gv3, n1, n2;
                tveq_out<MODE>(c.r.k[j], c.A[j], c1, c2, cx);
                tveq_adj(e1, e2, 0.f, 0.f, c.r.a1[j], c.r.a2[j], c.r.a3[j], q1, q2, gv3, n1, n2); e1 = n1; e2 = n2;
                tveq_adj(f1, f2, 0.f, 0.f, c.r.a1[j], c.r.a2[j], c.r.a3[j], q1, q2, gv3, n1, n2); f1 = n1; f2 = n2;
                tveq_adj(l1, l2, gv[j] * c1, gv[j] * c2, c.r.a1[j], c.r.a2[j], c.r.a3[j], q1, q2, gv3, n1, n2); l1 = n1; l2 = n2;
            }
            tv_scan(TvMap{e1, f1, e2, f2, l1, l2}, clam[par][0], clam[par][1], wt, l1, l2);
#pragma unroll
            for (int m = 0; m < TV_SPT; ++m) {
                const int j = TV_SPT - 1 - m;
                const float gyj = gv[j], k = c.r.k[j], A = c.A[j], gj = c.r.g[j], a1 = c.r.a1[j], a2 = c.r.a2[j], a3 = c.r.a3[j];
                float c1, c2, cx, q1, q2, gv3, n1, n2;
                tveq_out<MODE>(k, A, c1, c2, cx);
                tveq_adj(l1, l2, gyj * c1, gyj * c2, a1, a2, a3, q1, q2, gv3, n1, n2);
                s2[stage_word<TV_SPT>(i0 + j)] = MODE == TVEQ_HIGHSHELF ? __builtin_fmaf(gyj, cx, gv3) : gyj + gv3;
                const float v3 = xv[j] - zp2[j];
                const float v1 = __builtin_fmaf(a1, zp1[j], a2 * v3);                        // as tv_step had them
                const float v2 = zp2[j] + __builtin_fmaf(a2, zp1[j], a3 * v3);
                const float ga3 = q2 * v3;
                const float ga2 = __builtin_fmaf(gj, ga3, __builtin_fmaf(q1, v3, q2 * zp1[j]));
                const float ga1 = __builtin_fmaf(gj, ga2, q1 * zp1[j]);
                const float gd = -(a1 * a1) * ga1;                                           // 1 / a1 = 1 + g (g + k)
                float gg = __builtin_fmaf(a2, ga3, __builtin_fmaf(a1, ga2, (gj + gj + k) * gd));
                float dk, dA;
                if (MODE == TVEQ_BELL) {
                    dk = __builtin_fmaf(A, A, -1.f) * v1;
                    dA = 2.f * A * k * v1;
                } else if (MODE == TVEQ_LOWSHELF) {
                    dk = (A - 1.f) * v1;
                    dA = __builtin_fmaf(k, v1, 2.f * A * v2);
                } else {
                    dk = (1.f - A) * A * v1;
                    dA = __builtin_fmaf(2.f * A, xv[j] - v2, k * __builtin_fmaf(-2.f, A, 1.f) * v1);
                }
                float gk = __builtin_fmaf(gj, gd, gyj * dk);
                float gA = gyj * dA;
                if (!(t0 + i0 + j < N)) gg = gk = gA = 0.f;
                const float t = c.r.t[j], u = 1.f - t;
                p_gl = __builtin_fmaf(u, gg, p_gl);
                p_gr = __builtin_fmaf(t, gg, p_gr);
                p_kl = __builtin_fmaf(u, gk, p_kl);
                p_kr = __builtin_fmaf(t, gk, p_kr);
                p_al = __builtin_fmaf(u, gA, p_al);
                p_ar = __builtin_fmaf(t, gA, p_ar);
                l1 = n1;
                l2 = n2;
            }
            if (tid == TV_THREADS - 1) { clam[par ^ 1][0] = l1; clam[par ^ 1][1] = l2; }
        }
        {
            double d[6] = {(double)p_gl, (double)p_gr, (double)p_kl, (double)p_kr, (double)p_al, (double)p_ar};
            tv_group_sum(d, W);
            if ((tid & (W - 1)) == 0) {
                double* o = red[f / W];
#pragma unroll
                for (int i = 0; i < 6; ++i) o[i] = d[i];
            }
        }
        lds_barrier();
        // frame point i of the tile: the interval before it, then its own, then - on the tile's end - what the later tile carried
        for (int i = tid; i <= nint; i += TV_THREADS) {
            double sg = 0.0, sk = 0.0, sa = 0.0;
            if (i > 0)
                for (int s = 0; s < S; ++s) { sg += red[(i - 1) * S + s][1]; sk += red[(i - 1) * S + s][3]; sa += red[(i - 1) * S + s][5]; }
            if (i < nint)
                for (int s = 0; s < S; ++s) { sg += red[i * S + s][0]; sk += red[i * S + s][2]; sa += red[i * S + s][4]; }
            if (i == nint) { sg += edge[par][0]; sk += edge[par][1]; sa += edge[par][2]; }
            if (i == 0 && ti > 0) {
                edge[par ^ 1][0] = sg;
                edge[par ^ 1][1] = sk;
                edge[par ^ 1][2] = sa;
            } else if (j0 + i < F) {
                pr[j0 + i] = (float)sg;
                pr[F + j0 + i] = (float)sk;
                pr[2 * F + j0 + i] = (float)sa;
            }
        }
        if (gxr) {
            const int Tc = (int)min((long)TV_TILE, N - t0);
            for (int i = tid; i < Tc; i += TV_THREADS) st_stream(gxr + t0 + i, s2[stage_word<TV_SPT>(i)]);
        }
        lds_barrier();                                // red, s1, s2 and zin are written again by the next tile
        par ^= 1;
    }
}

// One thread per (item, frame point): its channels' sums in float64, channel by channel, then from (gG, gK, gA) to the three curves in
// float64 - G, K and A are functions of T = tan(..), Q and A that differ by mode - and exactly zero where the frame value was clamped.
__global__ void tveq_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ gain, const float* __restrict__ cut,
                                     const float* __restrict__ q, float* __restrict__ ggain, float* __restrict__ gcut, float* __restrict__ gq, int B, int C,
                                     long F, int mode, const TveqCfg g) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)B * F) return;
    const long b = id / F, j = id - b * F;
    const size_t stride = 3 * (size_t)F;
    double sg = 0.0, sk = 0.0, sa = 0.0;
    for (int c = 0; c < C; ++c) {
        const float* p = partials + ((size_t)b * C + c) * stride;
        sg += (double)p[j];
        sk += (double)p[F + j];
        sa += (double)p[2 * F + j];
    }
    const double av = (double)gain[id], cv = (double)cut[id], qv = (double)q[id];
    const TveqPoint p = tveq_point(av, cv, qv, mode, g);
    double gT, gQ, gA;
    if (mode == TVEQ_BELL) {                             // G = T, K = 1 / (Q A)
        gT = sg;
        gQ = -sk * p.K / p.Q;
        gA = sa - sk * p.K / p.A;
    } else {                                             // G = T / sqrt A or T sqrt A, K = 1 / Q
        const double r = sqrt(p.A), h = sg * p.G / (2.0 * p.A);
        gT = mode == TVEQ_LOWSHELF ? sg / r : sg * r;
        gQ = -sk / (p.Q * p.Q);
        gA = mode == TVEQ_LOWSHELF ? sa - h : sa + h;
    }
    ggain[id] = av < -TVEQ_DB_MAX || av > TVEQ_DB_MAX ? 0.f : (float)(gA * p.A * (2.302585092994046 / 40.0));
    gcut[id] = cv < g.flo || cv > g.fhi ? 0.f : (float)(gT * g.wk * (1.0 + p.T * p.T));
    gq[id] = qv < TVEQ_Q_LO || qv > TVEQ_Q_HI ? 0.f : (float)gQ;
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
int tveq_args(const float* x, const float* gain, const float* cut, const float* q, int B, int C, long N, int hop, int mode, double sample_rate) {
    if (!x || !gain || !cut || !q || B <= 0 || C <= 0 || N <= 0 || hop <= 0 || mode < 0 || mode > 2 || !(sample_rate > 0.0) ||
        !(sample_rate - sample_rate == 0.0))
        return DASP_ERR_ARG;
    if (!tv_hop_ok(hop) || (long)B * C > 0x7fffffffL || tv_ntile(N) > 0x3fffffffL || (long)B > 0x7fffffffL * 64 / tv_frames_of(N, hop))
        return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
inline TveqCfg tveq_cfg(double sample_rate, int hop) {
    int lg = 0;
    while ((1 << lg) < hop) ++lg;
    return TveqCfg{3.141592653589793 / sample_rate, sample_rate / 4096.0, 0.49 * sample_rate, 1.f / (float)hop, hop, lg};
}

template <int MODE>
void tveq_launch_forward(const float* x, const float* gain, const float* cut, const float* q, float* y, float* states, int B, int C, long N, long F,
                         const TveqCfg& g, hipStream_t st) {
    const dim3 grid((unsigned)((long)B * C)), block(TV_THREADS);
    const int nt = (int)tv_ntile(N);
    if (states) hipLaunchKernelGGL((tveq_forward_kernel<MODE, true>), grid, block, 0, st, x, gain, cut, q, y, states, N, nt, C, F, g);
    else hipLaunchKernelGGL((tveq_forward_kernel<MODE, false>), grid, block, 0, st, x, gain, cut, q, y, states, N, nt, C, F, g);
}
template <int MODE>
void tveq_launch_backward(const float* x, const float* gain, const float* cut, const float* q, const float* states, const float* gy, float* gx,
                          float* scratch, int B, int C, long N, long F, const TveqCfg& g, hipStream_t st) {
    hipLaunchKernelGGL(tveq_backward_kernel<MODE>, dim3((unsigned)((long)B * C)), dim3(TV_THREADS), 0, st, x, gain, cut, q, states, gy, gx, scratch, N,
                       (int)tv_ntile(N), C, F, g);
}
}  // namespace

extern "C" {

int dasp_tveq_tile(void) { return TV_TILE; }
long dasp_tveq_state_floats(long rows, long N) { return rows <= 0 || N <= 0 ? DASP_ERR_ARG : rows * tv_ntile(N) * 2; }
long dasp_tveq_scratch_floats(long rows, long N, int hop) {
    if (rows <= 0 || N <= 0 || hop <= 0) return DASP_ERR_ARG;
    return tv_hop_ok(hop) ? rows * 3 * tv_frames_of(N, hop) : DASP_ERR_UNSUPPORTED;
}

int dasp_tveq_forward(const float* x, const float* gain_db, const float* cutoff_hz, const float* q, float* y, float* states, int B, int C, long N, int hop,
                      int mode, double sample_rate, void* stream) {
    if (!y) return DASP_ERR_ARG;
    const int s = tveq_args(x, gain_db, cutoff_hz, q, B, C, N, hop, mode, sample_rate);
    if (s != DASP_OK) return s;
    const TveqCfg g = tveq_cfg(sample_rate, hop);
    const hipStream_t st = (hipStream_t)stream;
    const long F = tv_frames_of(N, hop);
    if (mode == TVEQ_BELL) tveq_launch_forward<TVEQ_BELL>(x, gain_db, cutoff_hz, q, y, states, B, C, N, F, g, st);
    else if (mode == TVEQ_LOWSHELF) tveq_launch_forward<TVEQ_LOWSHELF>(x, gain_db, cutoff_hz, q, y, states, B, C, N, F, g, st);
    else tveq_launch_forward<TVEQ_HIGHSHELF>(x, gain_db, cutoff_hz, q, y, states, B, C, N, F, g, st);
    return launch_status();
}

int dasp_tveq_backward(const float* x, const float* gain_db, const float* cutoff_hz, const float* q, const float* states, const float* gy, float* gx,
                       float* ggain, float* gcutoff, float* gq, float* scratch, int B, int C, long N, int hop, int mode, double sample_rate, void* stream) {
    if (!states || !gy || !ggain || !gcutoff || !gq || !scratch) return DASP_ERR_ARG;
    int s = tveq_args(x, gain_db, cutoff_hz, q, B, C, N, hop, mode, sample_rate);
    if (s != DASP_OK) return s;
    const TveqCfg g = tveq_cfg(sample_rate, hop);
    const hipStream_t st = (hipStream_t)stream;
    const long F = tv_frames_of(N, hop);
    if (mode == TVEQ_BELL) tveq_launch_backward<TVEQ_BELL>(x, gain_db, cutoff_hz, q, states, gy, gx, scratch, B, C, N, F, g, st);
    else if (mode == TVEQ_LOWSHELF) tveq_launch_backward<TVEQ_LOWSHELF>(x, gain_db, cutoff_hz, q, states, gy, gx, scratch, B, C, N, F, g, st);
    else tveq_launch_backward<TVEQ_HIGHSHELF>(x, gain_db, cutoff_hz, q, states, gy, gx, scratch, B, C, N, F, g, st);
    if ((s = launch_status()) != DASP_OK) return s;
    hipLaunchKernelGGL(tveq_finalize_kernel, dim3((unsigned)(((long)B * F + 127) / 128)), dim3(128), 0, st, (const float*)scratch, gain_db, cutoff_hz, q,
                       ggain, gcutoff, gq, B, C, F, mode, g);
    return launch_status();
}

}  // extern "C"
