// envelope_follower and gain_curve: the two control-rate side chains. audio -> curve and curve -> gain, one read pass each.
//
// ENVELOPE. For item b, with N = seq_len, h = hop, F = ceil(N / h) + 1 frame points, frame point j at sample j h, the level zero from
// sample N on and e[-1] = 0:
//   t = clamp(smoothing_ms, 0.1, 10000);   a = exp(-ln 9 / (sr t / 1000))
//   p[m] = max_c |x[b,c,m]| (peak; the lowest channel wins a tie, a NaN channel makes p NaN) | mean_c x[b,c,m]^2 (power)
//   e[m] = a e[m-1] + (1 - a) p[m];   E[b,j] = e[j h]
// a is constant per item, so the recurrence is not walked. With s = (j - 1) h:
//   E_j = a^h E_{j-1} + z_j,   z_j = sum_{i=1..h} (1 - a) a^(h-i) p[s+i],   E_0 = (1 - a) p[0]
//   D_j = dE_j/da = h a^(h-1) E_{j-1} + a^h D_{j-1} + dz_j,   dz_j = sum_i [-a^(h-i) + (1 - a)(h-i) a^(h-i-1)] p[s+i],   D_0 = -p[0]
// PASS 1 (envelope_block_kernel): one workgroup per (item, tile of 4096 samples from sample 4096 k + 1 on), all channels. p goes through
//   LDS (a lane per consecutive sample on the global side, 16 consecutive samples per thread on the other). A thread's 16 samples are two
//   runs of 8; a run that ends d0 samples before its block does contributes a^d0 sum_r w[r] p, w[r] = (1 - a) a^r for the sample r before
//   the run's end: two factors, each from float64 and rounded once (1 - a = -expm1(ln a)). The runs of a thread are added, then the
//   threads of a block on DPP row shifts and row broadcasts (hop 32 .. 1024), then two waves through LDS (hop 2048): one fixed order.
//   Nothing per sample is written: 4 C bytes per sample of traffic. dz_j is formed only when the tangent is asked for.
// PASS 2 (envelope_scan_kernel): one workgroup per item over the F values in float64: every thread walks a run of consecutive frames
//   from zero state, the runs' ends are scanned over the threads (eight doubling steps; a step over n frames multiplies by
//   [[a^(n h), 0], [n h a^(n h - 1), a^(n h)]], powers from exp(k ln a)), then every thread walks its run again from its true state.
// BACKWARD: g_smoothing = (da/dt) sum_j gE_j D_j, Lambda_j = gE_j + a^h Lambda_{j+1} by the same scan in reverse (envelope_adjoint_kernel,
//   one workgroup per item, float64), then one elementwise pass gx[b,c,m] = (1 - a) a^(j h - m) Lambda_j dp/dx, j = ceil(m / h)
//   (envelope_gx_kernel: reads x, writes gx, the winner found again by the forward pass's rule, the weight the same two factors).
//
// GAIN_CURVE. j = n / h, t = (n mod h) / h, g = P_j + t (P_{j+1} - P_j) in dB (P_j itself at t = 0, so that a NaN P_{j+1} does not
// reach sample j h), y = x exp(g ln 10 / 20). Backward: gx = gy G and, with q = (ln 10 / 20) sum_c gy x G, per interval
// A_j = sum (1 - t) q and B_j = sum t q - the same runs of 8, DPP and LDS order as above - written to scratch; a second small launch
// joins them, gP_j = A_j + B_{j-1}. Tiles of 4096 samples hold whole intervals, so tiles are independent in both directions.
//
// No atomics anywhere: every result is bit-identical run to run and for an item alone or in a batch.
#include "row_helpers.hpp"

namespace dasp {

constexpr int ENV_THREADS = 256;
constexpr int ENV_SPT = 16;                           // consecutive samples per thread
constexpr int ENV_TILE = ENV_THREADS * ENV_SPT;       // 4096: a multiple of every hop
constexpr int ENV_RUN = 8;                            // the smallest hop
constexpr int ENV_NW = ENV_THREADS / 64;
constexpr int ENV_STAGE = ENV_TILE + ENV_TILE / ENV_SPT;
constexpr float LN10_20 = 0.11512925464970229f;

__host__ __device__ inline bool env_hop_ok(int hop) { return hop >= 8 && hop <= 2048 && !(hop & (hop - 1)); }
__host__ __device__ inline long env_frames(long N, int hop) { return (N + hop - 1) / hop + 1; }

struct EnvItem { double lna, oma, t; float pois; bool clamped; };          // ln a, 1 - a
__device__ __forceinline__ EnvItem env_item(const float* __restrict__ ctl, int b, double sr) {
    const double r = (double)ctl[b];
    EnvItem it;
    it.clamped = r < 0.1 || r > 10000.0;
    it.t = r < 0.1 ? 0.1 : (r > 10000.0 ? 10000.0 : r);                     // a NaN stays
    it.lna = -2.1972245773362196 / (sr * it.t / 1000.0);
    it.oma = -expm1(it.lna);
    it.pois = r != r ? __builtin_nanf("") : 0.f;
    return it;
}
__device__ __forceinline__ double env_pow(double lna, long k) { return k == 0 ? 1.0 : exp((double)k * lna); }      // a^k; a may be 0

// v summed over groups of 2^k adjacent lanes, k = 0 .. 6, in the last lane of every group (the steps of wave_sum_uniform, cut short)
__device__ __forceinline__ float env_group_sum(float v, int k) {
    if (k >= 1) v += dpp_or_zero<0x111, 0xf>(v);       // row_shr:1
    if (k >= 2) v += dpp_or_zero<0x112, 0xf>(v);       // row_shr:2
    if (k >= 3) v += dpp_or_zero<0x114, 0xf>(v);       // row_shr:4
    if (k >= 4) v += dpp_or_zero<0x118, 0xf>(v);       // row_shr:8
    if (k >= 5) v += dpp_or_zero<0x142, 0xa>(v);       // row_bcast:15
    if (k >= 6) v += dpp_or_zero<0x143, 0xc>(v);       // row_bcast:31
    return v;
}

// Two values per thread and block-of-hop sums of them, hop >= 16: u[0], u[1] are what the thread's 16 samples give to the block they lie
// in. Writes o0[j], o1[j] (o1 may be null) for the blocks j0 + (block in tile) < jend. wred: 2 * ENV_NW floats of LDS.
__device__ __forceinline__ void env_block_store(float u0, float u1, bool two, float* __restrict__ o0, float* __restrict__ o1, long stride,
                                                long j0, long jend, int hop, float* wred, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    const int lpb = hop / ENV_SPT;                                        // threads per block
    const int k = 31 - __builtin_clz(lpb < 64 ? lpb : 64);
    u0 = env_group_sum(u0, k);
    if (two) u1 = env_group_sum(u1, k);
    if (lpb <= 64) {
        const long j = j0 + tid / lpb;
        if ((lane & (lpb - 1)) == lpb - 1 && j < jend) {
            o0[j * stride] = u0;
            if (two) o1[j * stride] = u1;
        }
        return;
    }
    if (lane == 63) { wred[wv] = u0; wred[ENV_NW + wv] = u1; }            // hop 2048: two waves per block
    __syncthreads();
    if (tid < ENV_NW / 2 && j0 + tid < jend) {
        o0[(j0 + tid) * stride] = wred[2 * tid] + wred[2 * tid + 1];
        if (two) o1[(j0 + tid) * stride] = wred[ENV_NW + 2 * tid] + wred[ENV_NW + 2 * tid + 1];
    }
}

template <bool PEAK> __device__ __forceinline__ float env_level(const float* __restrict__ xb, long N, int C, long m, float invC, int& cs) {
    const float v = xb[m];
    float p = PEAK ? fabsf(v) : v * v;
    cs = 0;
    for (int c = 1; c < C; ++c) {
        const float o = xb[(size_t)c * N + m];
        if (PEAK) {
            const float a = fabsf(o);
            if (a > p) { p = a; cs = c; } else if (a != a) p = a;
        } else
            p = __builtin_fmaf(o, o, p);
    }
    return PEAK ? p : p * invC;
}

template <bool PEAK, bool TAN>
__global__ void __launch_bounds__(ENV_THREADS)
envelope_block_kernel(const float* __restrict__ x, const float* __restrict__ ctl, float* __restrict__ z, float* __restrict__ dz, long N, long F,
                      int ntile, int C, int hop, double sr) {
    __shared__ float st[ENV_STAGE];
    __shared__ float wts[3][ENV_RUN];
    __shared__ float wred[2 * ENV_NW];
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const EnvItem it = env_item(ctl, b, sr);
    const float* xb = x + (size_t)b * C * N;
    const float invC = 1.f / (float)C;
    const long t0 = (long)tile * ENV_TILE + 1;                            // block j covers samples (j - 1) h + 1 .. j h

    if (tid < ENV_RUN) {                                                  // the sample r before a run's end
        const double ar = env_pow(it.lna, tid);
        wts[0][tid] = (float)(it.oma * ar);
        wts[1][tid] = (float)(-ar + (tid ? it.oma * (double)tid * env_pow(it.lna, tid - 1) : 0.0));
        wts[2][tid] = (float)ar;
    }
    float pk[ENV_SPT];
    stage_load<ENV_SPT, ENV_THREADS>(pk, xb, t0, N, tid);
#pragma unroll
    for (int m = 0; m < ENV_SPT; ++m) pk[m] = PEAK ? fabsf(pk[m]) : pk[m] * pk[m];
    for (int c = 1; c < C; ++c) {
        float o[ENV_SPT];
        stage_load<ENV_SPT, ENV_THREADS>(o, xb + (size_t)c * N, t0, N, tid);
#pragma unroll
        for (int m = 0; m < ENV_SPT; ++m) {
            if (PEAK) {
                const float a = fabsf(o[m]);
                if (a > pk[m] || a != a) pk[m] = a;
            } else
                pk[m] = __builtin_fmaf(o[m], o[m], pk[m]);
        }
    }
    if (!PEAK) {
#pragma unroll
        for (int m = 0; m < ENV_SPT; ++m) pk[m] *= invC;
    }
    stage_put<ENV_SPT, ENV_THREADS>(st, pk, tid);
    __syncthreads();

    float zq[2], dq[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int o = (ENV_SPT * tid + ENV_RUN * q) & (hop - 1), d0 = hop - o - ENV_RUN;
        float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int i = 0; i < ENV_RUN; ++i) {
            const float p = st[stage_word<ENV_SPT>(ENV_SPT * tid + ENV_RUN * q + i)];
            const int r = ENV_RUN - 1 - i;
            s1 = __builtin_fmaf(wts[0][r], p, s1);
            if (TAN) { s2 = __builtin_fmaf(wts[1][r], p, s2); s3 = __builtin_fmaf(wts[2][r], p, s3); }
        }
        const float a0 = (float)env_pow(it.lna, d0);
        zq[q] = a0 * s1;
        dq[q] = 0.f;
        if (TAN) {
            const float b0 = d0 ? (float)(it.oma * (double)d0 * env_pow(it.lna, d0 - 1)) : 0.f;
            dq[q] = a0 * s2 + b0 * s3;
        }
    }
    float* zb = z + (size_t)b * F;
    float* db = TAN ? dz + (size_t)b * F : nullptr;
    const long j0 = (long)tile * (ENV_TILE / hop) + 1;
    if (hop == ENV_RUN) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const long j = j0 + 2 * tid + q;
            if (j < F) { zb[j] = zq[q]; if (TAN) db[j] = dq[q]; }
        }
    } else
        env_block_store(zq[0] + zq[1], dq[0] + dq[1], TAN, zb, db, 1, j0, F, hop, wred, tid);
    if (tile == 0 && tid == 0) {                                          // frame point 0 is sample 0 alone
        int cs;
        const float p0 = env_level<PEAK>(xb, N, C, 0, invC, cs);
        zb[0] = (float)it.oma * p0;
        if (TAN) db[0] = -p0;
    }
}

// E_j = A E_{j-1} + z_j and D_j = Bc E_{j-1} + A D_{j-1} + dz_j over the F frames of an item, float64
template <bool TAN>
__global__ void __launch_bounds__(ENV_THREADS)
envelope_scan_kernel(const float* __restrict__ ctl, const float* __restrict__ z, const float* __restrict__ dz, float* __restrict__ E,
                     float* __restrict__ D, long F, int hop, double sr) {
    __shared__ double se[2][ENV_THREADS], sd[2][ENV_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const EnvItem it = env_item(ctl, b, sr);
    const double A = env_pow(it.lna, hop), Bc = (double)hop * env_pow(it.lna, hop - 1);
    const float* zb = z + (size_t)b * F;
    const float* db = TAN ? dz + (size_t)b * F : nullptr;
    const long L = (F - 1 + ENV_THREADS - 1) / ENV_THREADS;               // frames 1 .. F - 1 in runs of L
    const long j0 = 1 + (long)tid * L, j1 = j0 + L < F ? j0 + L : F;
    const double e00 = (double)zb[0], d00 = TAN ? (double)db[0] : 0.0;
    double e = tid ? 0.0 : e00, d = tid ? 0.0 : d00;
    for (long j = j0; j < j1; ++j) {
        if (TAN) d = Bc * e + A * d + (double)db[j];
        e = A * e + (double)zb[j];
    }
    int cur = 0;
    se[0][tid] = e; sd[0][tid] = d;
    __syncthreads();
    if (L > 0) {
        for (int s = 1; s < ENV_THREADS; s <<= 1) {
            double ne = se[cur][tid], nd = sd[cur][tid];
            if (tid >= s) {
                const long n = L * s * hop;
                const double P = env_pow(it.lna, n), Q = (double)n * env_pow(it.lna, n - 1), pe = se[cur][tid - s], pd = sd[cur][tid - s];
                ne += P * pe;
                if (TAN) nd += Q * pe + P * pd;
            }
            se[cur ^ 1][tid] = ne; sd[cur ^ 1][tid] = nd;
            __syncthreads();
            cur ^= 1;
        }
    }
    e = tid ? se[cur][tid - 1] : e00;
    d = tid ? sd[cur][tid - 1] : d00;
    float* Eb = E + (size_t)b * F;
    float* Db = TAN ? D + (size_t)b * F : nullptr;
    if (tid == 0) { Eb[0] = (float)e + it.pois; if (TAN) Db[0] = (float)d + it.pois; }
    for (long j = j0; j < j1; ++j) {
        if (TAN) d = Bc * e + A * d + (double)db[j];
        e = A * e + (double)zb[j];
        Eb[j] = (float)e + it.pois;
        if (TAN) Db[j] = (float)d + it.pois;
    }
}

// g_smoothing = (da/dt) sum_j gE_j D_j (gctl non-null) and Lambda_j = gE_j + A Lambda_{j+1} (lam non-null), float64
__global__ void __launch_bounds__(ENV_THREADS)
envelope_adjoint_kernel(const float* __restrict__ ctl, const float* __restrict__ gE, const float* __restrict__ D, float* __restrict__ lam,
                        float* __restrict__ gctl, long F, int hop, double sr) {
    __shared__ double sl[2][ENV_THREADS], red[ENV_NW];
    const int tid = threadIdx.x, b = blockIdx.x, lane = lane_id(), wv = wave_id();
    const EnvItem it = env_item(ctl, b, sr);
    const double A = env_pow(it.lna, hop);
    const float* gb = gE + (size_t)b * F;
    const long L = (F + ENV_THREADS - 1) / ENV_THREADS;                   // frames 0 .. F - 1 in runs of L
    const long j0 = (long)tid * L < F ? (long)tid * L : F, j1 = j0 + L < F ? j0 + L : F;
    if (gctl) {
        const float* Db = D + (size_t)b * F;
        double s = 0.0;
        for (long j = j0; j < j1; ++j) s += (double)gb[j] * (double)Db[j];
        s = wave_sum(s);
        if (lane == 0) red[wv] = s;
        __syncthreads();
        if (tid == 0) {
            double g = red[0];
            for (int u = 1; u < ENV_NW; ++u) g += red[u];
            const double a = exp(it.lna);
            gctl[b] = (it.clamped ? 0.f : (float)(g * a * 2.1972245773362196 * 1000.0 / (sr * it.t * it.t))) + it.pois;
        }
    }
    if (!lam) return;
    double v = 0.0;
    for (long j = j1 - 1; j >= j0; --j) v = (double)gb[j] + A * v;
    int cur = 0;
    sl[0][tid] = v;
    __syncthreads();
    for (int s = 1; s < ENV_THREADS; s <<= 1) {
        double nv = sl[cur][tid];
        if (tid + s < ENV_THREADS) nv += env_pow(it.lna, L * s * hop) * sl[cur][tid + s];
        sl[cur ^ 1][tid] = nv;
        __syncthreads();
        cur ^= 1;
    }
    v = tid + 1 < ENV_THREADS ? sl[cur][tid + 1] : 0.0;
    float* lb = lam + (size_t)b * F;
    for (long j = j1 - 1; j >= j0; --j) {
        v = (double)gb[j] + A * v;
        lb[j] = (float)v;
    }
}

template <bool PEAK>
__global__ void __launch_bounds__(ENV_THREADS)
envelope_gx_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ lam, float* __restrict__ gx, long N,
                   long F, int ntile, int C, int hop, double sr) {
    __shared__ float hi[2048 / ENV_RUN], lo[ENV_RUN];
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const EnvItem it = env_item(ctl, b, sr);
    const float* xb = x + (size_t)b * C * N;
    float* gb = gx + (size_t)b * C * N;
    const float* lb = lam + (size_t)b * F;
    const float invC = 1.f / (float)C;
    if (tid < hop / ENV_RUN) hi[tid] = (float)env_pow(it.lna, ENV_RUN * tid);
    if (tid < ENV_RUN) lo[tid] = (float)(it.oma * env_pow(it.lna, tid));
    __syncthreads();
    const int lh = 31 - __builtin_clz(hop);
#pragma unroll 4
    for (int k = 0; k < ENV_SPT; ++k) {
        const long m = (long)tile * ENV_TILE + tid + ENV_THREADS * k;
        if (m >= N) break;
        const long j = (m + hop - 1) >> lh;
        const int d = (int)(j * hop - m);
        const float g = hi[d >> 3] * lo[d & 7] * lb[j];
        int cs;
        if (PEAK) {
            env_level<true>(xb, N, C, m, invC, cs);
            for (int c = 0; c < C; ++c) {
                const float v = xb[(size_t)c * N + m];
                gb[(size_t)c * N + m] = c == cs ? (v > 0.f ? g : (v < 0.f ? -g : 0.f * g)) : 0.f * g;
            }
        } else {
            const float g2 = 2.f * invC * g;
            for (int c = 0; c < C; ++c) gb[(size_t)c * N + m] = g2 * xb[(size_t)c * N + m];
        }
    }
}

// ---- gain_curve -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gc_gain(const float* __restrict__ Pb, long n, int hop, int lh, float invh) {
    const long j = n >> lh;
    const float t = (float)(int)(n & (hop - 1)) * invh, p0 = Pb[j];
    const float g = t == 0.f ? p0 : p0 + t * (Pb[j + 1] - p0);
    return expf(g * LN10_20);
}

__global__ void __launch_bounds__(ENV_THREADS)
gaincurve_forward_kernel(const float* __restrict__ x, const float* __restrict__ P, float* __restrict__ y, long N, long F, int ntile, int C, int hop) {
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const float* xb = x + (size_t)b * C * N;
    float* yb = y + (size_t)b * C * N;
    const float* Pb = P + (size_t)b * F;
    const int lh = 31 - __builtin_clz(hop);
    const float invh = 1.f / (float)hop;
#pragma unroll 4
    for (int k = 0; k < ENV_SPT; ++k) {
        const long n = (long)tile * ENV_TILE + tid + ENV_THREADS * k;
        if (n >= N) break;
        const float G = gc_gain(Pb, n, hop, lh, invh);
        for (int c = 0; c < C; ++c) yb[(size_t)c * N + n] = xb[(size_t)c * N + n] * G;
    }
}

// gx = gy G; ab (non-null: the frame gradients are wanted) receives A_j and B_j of every interval as pairs, ab[2 (b F + j)]
__global__ void __launch_bounds__(ENV_THREADS)
gaincurve_backward_kernel(const float* __restrict__ x, const float* __restrict__ P, const float* __restrict__ gy, float* __restrict__ gx,
                          float* __restrict__ ab, long N, long F, int ntile, int C, int hop) {
    __shared__ float st[ENV_STAGE];
    __shared__ float wred[2 * ENV_NW];
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const float* xb = x + (size_t)b * C * N;
    const float* gyb = gy + (size_t)b * C * N;
    float* gxb = gx ? gx + (size_t)b * C * N : nullptr;
    const float* Pb = P + (size_t)b * F;
    const int lh = 31 - __builtin_clz(hop);
    const float invh = 1.f / (float)hop;
    float q[ENV_SPT];
#pragma unroll 4
    for (int k = 0; k < ENV_SPT; ++k) {
        const long n = (long)tile * ENV_TILE + tid + ENV_THREADS * k;
        float qv = 0.f;
        if (n < N) {
            const float G = gc_gain(Pb, n, hop, lh, invh);
            for (int c = 0; c < C; ++c) {
                const float g = gyb[(size_t)c * N + n];
                if (gxb) gxb[(size_t)c * N + n] = g * G;
                qv = __builtin_fmaf(g * xb[(size_t)c * N + n], G, qv);
            }
            qv *= LN10_20;
        }
        q[k] = qv;
    }
    if (!ab) return;
    stage_put<ENV_SPT, ENV_THREADS>(st, q, tid);
    __syncthreads();
    float aq[2], bq[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int i = 0; i < ENV_RUN; ++i) {
            const int w = ENV_SPT * tid + ENV_RUN * u + i;
            const float t = (float)(w & (hop - 1)) * invh, v = st[stage_word<ENV_SPT>(w)];
            sa = __builtin_fmaf(1.f - t, v, sa);
            sb = __builtin_fmaf(t, v, sb);
        }
        aq[u] = sa; bq[u] = sb;
    }
    float* abb = ab + 2 * (size_t)b * F;
    const long j0 = (long)tile * (ENV_TILE / hop);
    if (hop == ENV_RUN) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long j = j0 + 2 * tid + u;
            if (j < F - 1) { abb[2 * j] = aq[u]; abb[2 * j + 1] = bq[u]; }
        }
    } else
        env_block_store(aq[0] + aq[1], bq[0] + bq[1], true, abb, abb + 1, 2, j0, F - 1, hop, wred, tid);
}

__global__ void __launch_bounds__(ENV_THREADS)
gaincurve_join_kernel(const float* __restrict__ ab, float* __restrict__ gP, long F, long total) {
    const long i = (long)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (i >= total) return;
    const long j = i % F;
    const float a = j < F - 1 ? ab[2 * i] : 0.f, bb = j > 0 ? ab[2 * (i - 1) + 1] : 0.f;
    gP[i] = a + bb;
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
int env_args(const void* x, const void* ctl, int B, int C, long N, int hop) {
    if (!x || !ctl || B <= 0 || C <= 0 || N <= 0 || hop <= 0) return DASP_ERR_ARG;
    if (!env_hop_ok(hop)) return DASP_ERR_UNSUPPORTED;
    const long ntile = (N + ENV_TILE - 1) / ENV_TILE + 1;
    if (N > (1L << 40) || (long)B * ntile >= 0x7fffffffL || (long)B * env_frames(N, hop) >= (1L << 37)) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
inline bool env_rate_ok(double sr) { return sr > 0.0 && sr - sr == 0.0; }
}  // namespace

extern "C" {

int dasp_envelope_tile(void) { return ENV_TILE; }

long dasp_envelope_scratch_floats(long B, long N, int hop) {
    if (B <= 0 || N <= 0 || hop <= 0) return DASP_ERR_ARG;
    if (!env_hop_ok(hop)) return DASP_ERR_UNSUPPORTED;
    return 2 * B * env_frames(N, hop);
}

int dasp_envelope_forward(const float* x, const float* smoothing_ms, float* env, float* tangent, float* scratch, int B, int C, long N, int hop,
                          int detector, double sample_rate, void* stream) {
    if (!env || !scratch || detector < 0 || detector > 1 || !env_rate_ok(sample_rate)) return DASP_ERR_ARG;
    const int s = env_args(x, smoothing_ms, B, C, N, hop);
    if (s != DASP_OK) return s;
    const hipStream_t st = (hipStream_t)stream;
    const long F = env_frames(N, hop);
    const int ntile = (int)(((F - 1) * hop + ENV_TILE - 1) / ENV_TILE);
    float *z = scratch, *dz = scratch + (size_t)B * F;
    const dim3 grid((unsigned)(B * ntile)), block(ENV_THREADS);
#define DASP_ENV_BLOCK(PEAK, TAN) \
    hipLaunchKernelGGL((envelope_block_kernel<PEAK, TAN>), grid, block, 0, st, x, smoothing_ms, z, dz, N, F, ntile, C, hop, sample_rate)
    if (detector == 0) { if (tangent) DASP_ENV_BLOCK(true, true); else DASP_ENV_BLOCK(true, false); }
    else { if (tangent) DASP_ENV_BLOCK(false, true); else DASP_ENV_BLOCK(false, false); }
#undef DASP_ENV_BLOCK
    if (tangent)
        hipLaunchKernelGGL(envelope_scan_kernel<true>, dim3((unsigned)B), block, 0, st, smoothing_ms, z, dz, env, tangent, F, hop, sample_rate);
    else
        hipLaunchKernelGGL(envelope_scan_kernel<false>, dim3((unsigned)B), block, 0, st, smoothing_ms, z, dz, env, tangent, F, hop, sample_rate);
    return launch_status();
}

int dasp_envelope_backward(const float* x, const float* smoothing_ms, const float* tangent, const float* genv, float* gx, float* gsmoothing,
                           float* scratch, int B, int C, long N, int hop, int detector, double sample_rate, void* stream) {
    if (!genv || (!gx && !gsmoothing) || (gx && !scratch) || (tangent == nullptr) != (gsmoothing == nullptr) || detector < 0 || detector > 1 ||
        !env_rate_ok(sample_rate))
        return DASP_ERR_ARG;
    const int s = env_args(x, smoothing_ms, B, C, N, hop);
    if (s != DASP_OK) return s;
    const hipStream_t st = (hipStream_t)stream;
    const long F = env_frames(N, hop);
    const dim3 block(ENV_THREADS);
    float* lam = gx ? scratch : nullptr;
    hipLaunchKernelGGL(envelope_adjoint_kernel, dim3((unsigned)B), block, 0, st, smoothing_ms, genv, tangent, lam, gsmoothing, F, hop, sample_rate);
    if (gx) {
        const int ntile = (int)((N + ENV_TILE - 1) / ENV_TILE);
        const dim3 grid((unsigned)(B * ntile));
        if (detector == 0)
            hipLaunchKernelGGL(envelope_gx_kernel<true>, grid, block, 0, st, x, smoothing_ms, lam, gx, N, F, ntile, C, hop, sample_rate);
        else
            hipLaunchKernelGGL(envelope_gx_kernel<false>, grid, block, 0, st, x, smoothing_ms, lam, gx, N, F, ntile, C, hop, sample_rate);
    }
    return launch_status();
}

long dasp_gaincurve_scratch_floats(long B, long N, int hop) { return dasp_envelope_scratch_floats(B, N, hop); }

int dasp_gaincurve_forward(const float* x, const float* gain_db, float* y, int B, int C, long N, int hop, void* stream) {
    if (!y) return DASP_ERR_ARG;
    const int s = env_args(x, gain_db, B, C, N, hop);
    if (s != DASP_OK) return s;
    const int ntile = (int)((N + ENV_TILE - 1) / ENV_TILE);
    hipLaunchKernelGGL(gaincurve_forward_kernel, dim3((unsigned)(B * ntile)), dim3(ENV_THREADS), 0, (hipStream_t)stream, x, gain_db, y, N,
                       env_frames(N, hop), ntile, C, hop);
    return launch_status();
}

int dasp_gaincurve_backward(const float* x, const float* gain_db, const float* gy, float* gx, float* ggain, float* scratch, int B, int C, long N,
                            int hop, void* stream) {
    if (!gy || (!gx && !ggain) || (ggain && !scratch)) return DASP_ERR_ARG;
    const int s = env_args(x, gain_db, B, C, N, hop);
    if (s != DASP_OK) return s;
    const hipStream_t st = (hipStream_t)stream;
    const long F = env_frames(N, hop);
    const int ntile = (int)((N + ENV_TILE - 1) / ENV_TILE);
    hipLaunchKernelGGL(gaincurve_backward_kernel, dim3((unsigned)(B * ntile)), dim3(ENV_THREADS), 0, st, x, gain_db, gy, gx, ggain ? scratch : nullptr,
                       N, F, ntile, C, hop);
    if (ggain) {
        const long total = (long)B * F;
        hipLaunchKernelGGL(gaincurve_join_kernel, dim3((unsigned)((total + ENV_THREADS - 1) / ENV_THREADS)), dim3(ENV_THREADS), 0, st, scratch, ggain, F,
                           total);
    }
    return launch_status();
}

}  // extern "C"
