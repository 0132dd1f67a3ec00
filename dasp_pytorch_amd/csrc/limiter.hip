// limiter: look-ahead brickwall limiter - the first scan of the library over the (max, x) semiring.
//
// For item b, with N = seq_len, L the look-ahead in samples and an internal timeline m in [0, N + L); everything before 0 and the level
// from N on are zero:
//   thr = clamp(threshold_db, -120, 40);   t = clamp(release_ms, 0.1, 10000);   rho = exp(-ln 9 / (sr t / 1000))
//   p[m] = max_c |x[b,c,m]|                                 (channels linked; the lowest channel wins a tie)
//   r[m] = max(0, 20 log10(max(p[m], eps)) - thr)           (required reduction in dB)
//   h[m] = max_{0<=k<=L} r[m-k]                             (hold; the latest sample wins a tie)
//   e[m] = max(h[m], rho e[m-1])                            (release; h wins a tie)   winner w[m]: the j with e[m] = rho^max(0,m-j-L) r[j]
//   s[m] = (1/(L+1)) sum_{j=0..L} e[m-j]                    (attack: a box of the look-ahead's length, in dB)
//   G[m] = 10^(-s[m]/20);   y[b,c,n] = x[b,c,n] G[n+L]
// Every e[n+L-j], 0 <= j <= L, is at least r[n], so s[n+L] >= r[n] and |y| <= 10^(thr/20).
//
// ONE WORKGROUP OWNS ONE ITEM, reads all its channels and walks the timeline in tiles of T = 2048 samples with the L samples before the
// tile (r and e of the tile before) kept in LDS; 512 threads, 4 consecutive samples each in the scans. Per tile:
//   1  r of the tile, a lane per consecutive sample on the global side, as 64-bit keys (bits of r | sample index): r >= 0, so the
//      unsigned maximum of two keys is the larger r and, of two equal r, the later sample - value and winner in one compare;
//   2  the hold: a log-step windowed maximum over tile + halo in LDS, floor(log2(L+1)) doubling passes and one pass that joins two
//      windows of 2^k to one of L + 1;
//   3  the release: thread tid takes the 4 consecutive samples from 4 tid on; the recurrence from zero state, then the scan of the
//      pairs (value, winner) over the lanes of a wave (six shuffles; a step over d lanes multiplies by rho^(4 d)) and over the eight
//      waves through LDS, then the fix-up e = max(local, rho^(j+1) carry). The powers of rho come from exp(k ln rho) in float64, rounded
//      once: a value that decays over k samples is rounded O(log k) times, not k times. One float and one index are carried per tile;
//   4  the box: a float64 prefix sum over tile + halo (6 consecutive samples per thread, the same two-level scan), s = (P[i] - P[i-L-1])
//      / (L+1): windows of zeros give exactly 0, and G = exp(-s ln 10 / 20) in float64 is exactly 1 there;
//   5  y = x G, a lane per consecutive sample, and with SAVE G[n+L] and w[n+L] for n in [0, N): 8 bytes per sample of the item.
// r = (float)(20 log10((double) p) - thr): float64 up to the one rounding, so that the ceiling is missed by roundings of r, G and the
// product alone.
//
// Backward, the same walk from the last tile; with q[n] = sum_c gy x G[n+L]:
//   ge[m] = -(ln 10 / 20) / (L+1) sum_{n=m-L..m} q[n]       (the box's adjoint, a prefix sum over tile + halo of q again)
//   k[m] = max(0, m - w[m] - L);   gr[j] = sum_{m: w[m]=j} rho^k ge[m];   B[j] = sum_{m: w[m]=j} k rho^(k-1) ge[m]
//   g_threshold_db = -sum_m rho^k ge[m];   g_rho = sum_j r[j] B[j];   gx[c,j] = gy G[j+L] + [c = c*] sign(x) gr[j] 20 / (ln 10 p[j])
// w is non-decreasing (underflow of e to zero apart, whose samples carry no gradient), so the m of one j are one run: a segmented sum
// in reverse time - thread r takes the run of thread 511 - r, last sample first - over triples (first key, last key, sum of the last
// key's run), associative; the open run is carried across tiles (one key, two floats). The head of a run - its earliest m - writes the
// two sums to scratch[j], j <= m: an address that this workgroup reaches, tile [j / T], in this step or a later one, after a barrier.
// The scratch is zeroed by a kernel in front. w[m] for m < L is not saved: there e = h is a running maximum, and the first tile runs
// the hold on r again. Control sums are float32 per thread and tile, float64 across tiles and the workgroup in a fixed order; the
// workgroup's tail applies the chain rule. No atomics: every result is bit-identical run to run and for an item alone or in a batch.
//
// Non-finite input: comparisons decide. A NaN peak gives r = 0 (the sample itself stays NaN in y), an inf peak r = inf, G = 0 from there
// on and NaN where it multiplies inf. A NaN control makes G, y and every gradient of its item NaN. The winners are indices that
// comparisons chose; what the backward kernel reads from `winner` is checked against [0, N) before it forms an address.
// LDS: 92 KiB, dynamic, the limit raised once per device. One workgroup per item: 16 items use 16 of 256 CUs. 512 threads
// of 4 samples, not 256 of 8: two waves per SIMD hide some of each other's float64 latencies (2.64 -> 1.75 ms forward + backward at
// (16,2,131072)); 1024 of 2 spills in the backward kernel.
#include <atomic>

#include "row_helpers.hpp"

namespace dasp {

constexpr int LIM_THREADS = 512;
constexpr int LIM_SPT = 4;
constexpr int LIM_TILE = LIM_THREADS * LIM_SPT;
constexpr int LIM_LMAX = 1024;
constexpr int LIM_BUF = LIM_TILE + LIM_LMAX;
constexpr int LIM_PPT = LIM_BUF / LIM_THREADS;       // consecutive positions per thread in the prefix sum
constexpr int LIM_NW = LIM_THREADS / 64;
typedef unsigned long long lim_key_t;

struct LimLds {
    lim_key_t ka[LIM_BUF], kb[LIM_BUF];
    double P[LIM_BUF];
    float eb[LIM_BUF];                                // forward: e; backward: q
    int wb[LIM_TILE];
    double wred[LIM_NW], red[LIM_NW][2];
    float wv[LIM_NW], cv[2], as[LIM_NW][2], ca[2], cb[2];
    int wi[LIM_NW], ci[2], ak[LIM_NW][2], ck[2], wprev;
};

struct LimItem { double lrho, t; float thr, rho, pois; bool cthr, crel; };

__device__ __forceinline__ LimItem lim_item(const float* __restrict__ ctl, int b, double sr) {
    const float a = ctl[2 * (size_t)b], r = ctl[2 * (size_t)b + 1];
    LimItem it;
    it.cthr = a < -120.f || a > 40.f;
    it.thr = a < -120.f ? -120.f : (a > 40.f ? 40.f : a);                 // a NaN stays
    const double rd = (double)r;
    it.crel = rd < 0.1 || rd > 10000.0;
    it.t = rd < 0.1 ? 0.1 : (rd > 10000.0 ? 10000.0 : rd);
    it.lrho = -2.1972245773362196 / (sr * it.t / 1000.0);
    it.rho = (float)exp(it.lrho);
    it.pois = (a != a || r != r) ? __builtin_nanf("") : 0.f;
    return it;
}

__device__ __forceinline__ void lim_barrier() { __syncthreads(); }

// the linked peak of sample n and the channel that has it
__device__ __forceinline__ float lim_peak(const float* __restrict__ xb, long N, int C, long n, int& cs) {
    float p = fabsf(xb[n]);
    cs = 0;
    for (int c = 1; c < C; ++c) {
        const float a = fabsf(xb[(size_t)c * N + n]);
        if (a > p) { p = a; cs = c; }
    }
    return p;
}
__device__ __forceinline__ float lim_r(float p, float eps, float thr) {
    const float pe = p < eps ? eps : p;
    const float d = (float)(20.0 * log10((double)pe) - (double)thr);
    return d > 0.f ? d : 0.f;                                               // a NaN is no reduction
}
__device__ __forceinline__ lim_key_t lim_key(float r, long m) {
    return ((lim_key_t)__float_as_uint(r) << 32) | (lim_key_t)(unsigned)(m + LIM_LMAX);
}
__device__ __forceinline__ float lim_key_val(lim_key_t k) { return __uint_as_float((unsigned)(k >> 32)); }
__device__ __forceinline__ int lim_key_idx(lim_key_t k) { return (int)(unsigned)k - LIM_LMAX; }

// keys of the positions [0, L + T) of the tile from t0: the halo is given, the tile's r comes from x
__device__ __forceinline__ void lim_tile_keys(lim_key_t* ka, const float* __restrict__ xb, long N, int C, long t0, int L, float eps, float thr, int tid) {
#pragma unroll
    for (int k = 0; k < LIM_SPT; ++k) {
        const int mi = tid + LIM_THREADS * k;
        const long m = t0 + mi;
        float r = 0.f;
        if (m < N) { int cs; r = lim_r(lim_peak(xb, N, C, m, cs), eps, thr); }
        ka[L + mi] = lim_key(r, m);
    }
}

// Windowed maximum over the L + 1 keys up to each position of [0, L + T). Call after a barrier; ends with one. Returns the buffer.
__device__ __forceinline__ lim_key_t* lim_hold(lim_key_t* a, lim_key_t* b, int L, int tid) {
    const int W = L + 1, cnt = L + LIM_TILE;
    if (W == 1) return a;
    const int kk = 31 - __builtin_clz(W);
    lim_key_t *src = a, *dst = b;
    for (int d = 0; d <= kk; ++d) {
        const int sh = d < kk ? (1 << d) : W - (1 << kk);
        if (sh == 0) break;
        for (int i = tid; i < cnt; i += LIM_THREADS) {
            lim_key_t v = src[i];
            if (i >= sh) { const lim_key_t o = src[i - sh]; if (o > v) v = o; }
            dst[i] = v;
        }
        lim_barrier();
        lim_key_t* t = src; src = dst; dst = t;
    }
    return src;
}

// P[i] = sum of src[0 .. i] in float64 for i < cnt. Call after a barrier; ends with one.
__device__ __forceinline__ void lim_prefix(const float* src, double* P, int cnt, double* wred, int tid) {
    const int lane = lane_id(), wv = wave_id();
    double v[LIM_PPT], run = 0.0;
#pragma unroll
    for (int j = 0; j < LIM_PPT; ++j) {
        const int i = LIM_PPT * tid + j;
        run += i < cnt ? (double)src[i] : 0.0;
        v[j] = run;
    }
    double inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    double base = __shfl_up(inc, 1, 64);
    if (lane == 0) base = 0.0;
    if (lane == 63) wred[wv] = inc;
    lim_barrier();
    for (int u = 0; u < wv; ++u) base += wred[u];
#pragma unroll
    for (int j = 0; j < LIM_PPT; ++j) {
        const int i = LIM_PPT * tid + j;
        if (i < cnt) P[i] = base + v[j];
    }
    lim_barrier();
}

template <bool SAVE>
__global__ void __launch_bounds__(LIM_THREADS)
limiter_forward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, float* __restrict__ y, float* __restrict__ gain,
                       int* __restrict__ win, long N, int ntile, int C, int L, double sr, float eps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lim_raw[];
    LimLds& s = *reinterpret_cast<LimLds*>(lim_raw);
    const int b = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const LimItem it = lim_item(ctl, b, sr);
    const float* xb = x + (size_t)b * C * N;
    float* yb = y + (size_t)b * C * N;
    const float rho = it.rho;
    float q[LIM_SPT], pw[6];
#pragma unroll
    for (int j = 0; j < LIM_SPT; ++j) q[j] = (float)exp((double)(j + 1) * it.lrho);
#pragma unroll
    for (int d = 0; d < 6; ++d) pw[d] = (float)exp((double)(LIM_SPT << d) * it.lrho);
    const float pwave = (float)exp((double)(64 * LIM_SPT) * it.lrho), plane = (float)exp((double)(LIM_SPT * lane) * it.lrho);
    const double invW = 1.0 / (double)(L + 1);

    for (int i = tid; i < L; i += LIM_THREADS) { s.ka[i] = lim_key(0.f, (long)i - L); s.eb[i] = 0.f; }
    if (tid == 0) { s.cv[0] = 0.f; s.ci[0] = -1; }
    int par = 0;
    for (int ti = 0; ti < ntile; ++ti, par ^= 1) {
        const long t0 = (long)ti * LIM_TILE;
        lim_tile_keys(s.ka, xb, N, C, t0, L, eps, it.thr, tid);
        lim_barrier();
        lim_key_t hk[LIM_LMAX / LIM_THREADS];                             // the next tile's halo, before the hold overwrites it
#pragma unroll
        for (int k = 0; k < LIM_LMAX / LIM_THREADS; ++k) {
            const int i = tid + LIM_THREADS * k;
            hk[k] = i < L ? s.ka[LIM_TILE + i] : 0ull;
        }
        const lim_key_t* H = lim_hold(s.ka, s.kb, L, tid);

        // release: the recurrence over the thread's samples from zero state, the scan of (value, winner), the fix-up
        float loc[LIM_SPT], ev = 0.f;
        int li[LIM_SPT], ei = -1;
        const int i0 = L + LIM_SPT * tid;
#pragma unroll
        for (int j = 0; j < LIM_SPT; ++j) {
            const lim_key_t key = H[i0 + j];
            const float hv = lim_key_val(key), c = rho * ev;
            if (c > hv) ev = c; else { ev = hv; ei = lim_key_idx(key); }
            loc[j] = ev; li[j] = ei;
        }
        float av = ev;
        int ai = ei;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const float lv = __shfl_up(av, 1 << d, 64);
            const int lw = __shfl_up(ai, 1 << d, 64);
            const float c = pw[d] * lv;
            if (lane >= (1 << d) && c > av) { av = c; ai = lw; }
        }
        float xv = __shfl_up(av, 1, 64);
        int xi = __shfl_up(ai, 1, 64);
        if (lane == 0) { xv = 0.f; xi = -1; }
        if (lane == 63) { s.wv[wv] = av; s.wi[wv] = ai; }
        lim_barrier();
        float cv = s.cv[par];
        int ci = s.ci[par];
        for (int u = 0; u < wv; ++u) {
            const float c = pwave * cv, tv = s.wv[u];
            if (c > tv) cv = c; else { cv = tv; ci = s.wi[u]; }
        }
        {
            const float c = plane * cv;
            if (c > xv) cv = c; else { cv = xv; ci = xi; }
        }
#pragma unroll
        for (int j = 0; j < LIM_SPT; ++j) {
            const float c = q[j] * cv;
            float e = loc[j];
            int w = li[j];
            if (c > e) { e = c; w = ci; }
            s.eb[i0 + j] = e;
            s.wb[LIM_SPT * tid + j] = e > 0.f ? w : -1;
            if (j == LIM_SPT - 1 && tid == LIM_THREADS - 1) { s.cv[par ^ 1] = e; s.ci[par ^ 1] = w; }
        }
        lim_barrier();
        lim_prefix(s.eb, s.P, L + LIM_TILE, s.wred, tid);

#pragma unroll
        for (int k = 0; k < LIM_SPT; ++k) {
            const int mi = tid + LIM_THREADS * k;
            const long n = t0 + mi - L;
            if (n >= 0 && n < N) {
                double sd = (s.P[mi + L] - (mi ? s.P[mi - 1] : 0.0)) * invW;
                sd = sd < 0.0 ? 0.0 : sd;
                const float G = (float)exp(-0.11512925464970229 * sd) + it.pois;
                for (int c = 0; c < C; ++c) yb[(size_t)c * N + n] = xb[(size_t)c * N + n] * G;
                if (SAVE) { gain[(size_t)b * N + n] = G; win[(size_t)b * N + n] = s.wb[mi]; }
            }
        }
        // the halo of the next tile: r as saved, e from the end of this tile (disjoint from what is written: L <= T)
#pragma unroll
        for (int k = 0; k < LIM_LMAX / LIM_THREADS; ++k) {
            const int i = tid + LIM_THREADS * k;
            if (i < L) { s.ka[i] = hk[k]; s.eb[i] = s.eb[LIM_TILE + i]; }
        }
    }
}

struct LimAgg { int first, last; float sa, sb; };
__device__ __forceinline__ void lim_join(int& last, float& sa, float& sb, const LimAgg& r) {       // (.., last, sums) then r
    const bool one = r.first == r.last && last == r.last;
    sa = one ? sa + r.sa : r.sa;
    sb = one ? sb + r.sb : r.sb;
    last = r.last;
}

__global__ void __launch_bounds__(LIM_THREADS)
limiter_backward_kernel(const float* __restrict__ x, const float* __restrict__ ctl, const float* __restrict__ gain, const int* __restrict__ win,
                        const float* __restrict__ gy, float* __restrict__ gx, float* __restrict__ gctl, f2* scratch, long N, int ntile, int C,
                        int L, double sr, float eps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lim_raw[];
    LimLds& s = *reinterpret_cast<LimLds*>(lim_raw);
    const int b = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const LimItem it = lim_item(ctl, b, sr);
    const float* xb = x + (size_t)b * C * N;
    const float* gb = gy + (size_t)b * C * N;
    const float* Gb = gain + (size_t)b * N;
    const int* wsv = win + (size_t)b * N;
    float* gxb = gx ? gx + (size_t)b * C * N : nullptr;
    f2* scr = scratch + (size_t)b * N;
    const double cW = -0.11512925464970229 / (double)(L + 1), invrho = exp(-it.lrho);

    if (tid == 0) { s.ck[0] = -1; s.ca[0] = 0.f; s.cb[0] = 0.f; }
    double s_thr = 0.0, s_rho = 0.0;
    int par = 0;
    for (int ti = ntile - 1; ti >= 0; --ti, par ^= 1) {
        const long t0 = (long)ti * LIM_TILE;
        // q over halo + tile, position i is sample n = t0 - L + i; w of the tile
        for (int i = tid; i < L + LIM_TILE; i += LIM_THREADS) {
            const long n = t0 - L + i;
            float qv = 0.f;
            if (n >= 0 && n < N) {
                const float g = Gb[n];
                for (int c = 0; c < C; ++c) qv = __builtin_fmaf(gb[(size_t)c * N + n] * xb[(size_t)c * N + n], g, qv);
            }
            s.eb[i] = qv;
        }
#pragma unroll
        for (int k = 0; k < LIM_SPT; ++k) {
            const int mi = tid + LIM_THREADS * k;
            const long m = t0 + mi;
            if (m >= L) s.wb[mi] = m - L < N ? wsv[m - L] : -1;
        }
        if (tid == 0) s.wprev = (t0 > 0 && t0 - 1 - L < N) ? wsv[t0 - 1 - L] : -1;       // t0 > 0: t0 - 1 >= L
        if (ti == 0 && L > 0) {                                                // w[m], m < L: the hold of the first tile again
            for (int i = tid; i < L; i += LIM_THREADS) s.ka[i] = lim_key(0.f, (long)i - L);
            lim_tile_keys(s.ka, xb, N, C, 0, L, eps, it.thr, tid);
            lim_barrier();
            const lim_key_t* H = lim_hold(s.ka, s.kb, L, tid);
            for (int mi = tid; mi < L; mi += LIM_THREADS) {
                const lim_key_t key = H[L + mi];
                s.wb[mi] = lim_key_val(key) > 0.f ? lim_key_idx(key) : -1;
            }
        }
        lim_barrier();
        lim_prefix(s.eb, s.P, L + LIM_TILE, s.wred, tid);

        // reverse time: thread tid has the run of thread 255 - tid, last sample first
        int key[LIM_SPT];
        float a[LIM_SPT], bb[LIM_SPT], t_thr = 0.f;
        const int u0 = LIM_SPT * tid;
#pragma unroll
        for (int j = 0; j < LIM_SPT; ++j) {
            const int mi = LIM_TILE - 1 - u0 - j;
            const long m = t0 + mi;
            const int w = s.wb[mi];
            const bool valid = w >= 0 && w < N;
            const double ge = cW * (s.P[mi + L] - (mi ? s.P[mi - 1] : 0.0));
            long kd = m - w - L;
            kd = kd < 0 ? 0 : kd;
            const double pk = exp((double)kd * it.lrho);
            key[j] = valid ? w : -1;
            a[j] = valid ? (float)(pk * ge) : 0.f;
            bb[j] = valid && kd > 0 ? (float)((double)kd * pk * invrho * ge) : 0.f;
            t_thr -= a[j];
        }
        LimAgg g{key[0], key[0], a[0], bb[0]};
#pragma unroll
        for (int j = 1; j < LIM_SPT; ++j) {
            if (key[j] == g.last) { g.sa += a[j]; g.sb += bb[j]; } else { g.last = key[j]; g.sa = a[j]; g.sb = bb[j]; }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            LimAgg o;
            o.first = __shfl_up(g.first, d, 64); o.last = __shfl_up(g.last, d, 64);
            o.sa = __shfl_up(g.sa, d, 64); o.sb = __shfl_up(g.sb, d, 64);
            if (lane >= d) {
                lim_join(o.last, o.sa, o.sb, g);
                g.first = o.first; g.last = o.last; g.sa = o.sa; g.sb = o.sb;
            }
        }
        LimAgg ex;
        ex.first = __shfl_up(g.first, 1, 64); ex.last = __shfl_up(g.last, 1, 64);
        ex.sa = __shfl_up(g.sa, 1, 64); ex.sb = __shfl_up(g.sb, 1, 64);
        if (lane == 63) { s.ak[wv][0] = g.first; s.ak[wv][1] = g.last; s.as[wv][0] = g.sa; s.as[wv][1] = g.sb; }
        lim_barrier();
        int cur = s.ck[par];
        float sa = s.ca[par], sb = s.cb[par];
        for (int u = 0; u < wv; ++u) lim_join(cur, sa, sb, LimAgg{s.ak[u][0], s.ak[u][1], s.as[u][0], s.as[u][1]});
        if (lane > 0) lim_join(cur, sa, sb, ex);
#pragma unroll
        for (int j = 0; j < LIM_SPT; ++j) {
            const int mi = LIM_TILE - 1 - u0 - j;
            if (key[j] == cur) { sa += a[j]; sb += bb[j]; } else { cur = key[j]; sa = a[j]; sb = bb[j]; }
            int nk;                                                        // the key of the sample before
            if (j < LIM_SPT - 1) nk = key[j + 1];
            else {
                const int w = mi ? s.wb[mi - 1] : s.wprev;
                nk = w >= 0 && w < N ? w : -1;
            }
            const bool head = nk != cur;
            if (head && cur >= 0) scr[cur] = f2{sa, sb};
            if (mi == 0) { s.ck[par ^ 1] = head ? -1 : cur; s.ca[par ^ 1] = head ? 0.f : sa; s.cb[par ^ 1] = head ? 0.f : sb; }
        }
        s_thr += (double)t_thr;
        __threadfence_block();
        lim_barrier();

        // the samples j of the tile: every run that names them has written
        float t_rho = 0.f;
#pragma unroll
        for (int k = 0; k < LIM_SPT; ++k) {
            const long j = t0 + tid + LIM_THREADS * k;
            if (j < N) {
                const f2 ab = scr[j];
                int cs;
                const float p = lim_peak(xb, N, C, j, cs), r = lim_r(p, eps, it.thr), G = Gb[j];
                const bool lim = r > 0.f;
                if (lim) t_rho = __builtin_fmaf(r, ab.y, t_rho);
                if (gxb) {
                    for (int c = 0; c < C; ++c) {
                        float v = gb[(size_t)c * N + j] * G;
                        if (lim && c == cs) {
                            const float xv = xb[(size_t)c * N + j];
                            v += (xv < 0.f ? -ab.x : ab.x) * (8.685889638065037f / p);
                        }
                        gxb[(size_t)c * N + j] = v;
                    }
                }
            }
        }
        s_rho += (double)t_rho;
    }
    s_thr = wave_sum(s_thr);
    s_rho = wave_sum(s_rho);
    if (lane == 0) { s.red[wv][0] = s_thr; s.red[wv][1] = s_rho; }
    lim_barrier();
    if (tid == 0) {
        double gt = s.red[0][0], gr = s.red[0][1];
        for (int u = 1; u < LIM_NW; ++u) { gt += s.red[u][0]; gr += s.red[u][1]; }
        const double rho = exp(it.lrho);
        const float o0 = it.cthr ? 0.f : (float)gt;
        const float o1 = it.crel ? 0.f : (float)(gr * rho * 2.1972245773362196 * 1000.0 / (sr * it.t * it.t));
        gctl[2 * (size_t)b] = o0 + it.pois;
        gctl[2 * (size_t)b + 1] = o1 + it.pois;
    }
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline long lim_ntile(long N, int L) { return (N + L + LIM_TILE - 1) / LIM_TILE; }

int lim_prepare() {
    static std::atomic<bool> asked[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (dev >= 0 && dev < 64 && asked[dev].load(std::memory_order_acquire)) return DASP_OK;
    const void* fns[3] = {reinterpret_cast<const void*>(limiter_forward_kernel<false>), reinterpret_cast<const void*>(limiter_forward_kernel<true>),
                          reinterpret_cast<const void*>(limiter_backward_kernel)};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LimLds));
        if (e != hipSuccess) return (int)e;
    }
    if (dev >= 0 && dev < 64) asked[dev].store(true, std::memory_order_release);
    return DASP_OK;
}

int lim_args(const float* x, const float* ctl, int B, int C, long N, int L, double sample_rate, double eps) {
    if (!x || !ctl || B <= 0 || C <= 0 || N <= 0 || L < 0 || !(sample_rate > 0.0) || !(sample_rate - sample_rate == 0.0) || !(eps >= 0.0) ||
        !(eps - eps == 0.0))
        return DASP_ERR_ARG;
    if (L > LIM_LMAX || N > 0x7fffffffL - 2 * LIM_LMAX - LIM_TILE) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
}  // namespace

extern "C" {

int dasp_limiter_tile(void) { return LIM_TILE; }
int dasp_limiter_max_lookahead(void) { return LIM_LMAX; }
long dasp_limiter_state_floats(long B, long N) { return B <= 0 || N <= 0 ? DASP_ERR_ARG : 2 * B * N; }
long dasp_limiter_partial_floats(long B, long N) { return B <= 0 || N <= 0 ? DASP_ERR_ARG : 2 * B * N; }
int dasp_limiter_prepare(void) { return lim_prepare(); }

int dasp_limiter_forward(const float* x, const float* ctl, float* y, float* gain, int* winner, int B, int C, long N, int lookahead,
                         double sample_rate, double eps, void* stream) {
    if (!y || (gain == nullptr) != (winner == nullptr)) return DASP_ERR_ARG;
    int s = lim_args(x, ctl, B, C, N, lookahead, sample_rate, eps);
    if (s != DASP_OK) return s;
    if ((s = lim_prepare()) != DASP_OK) return s;
    const dim3 grid((unsigned)B), block(LIM_THREADS);
    const int nt = (int)lim_ntile(N, lookahead);
    if (gain)
        hipLaunchKernelGGL(limiter_forward_kernel<true>, grid, block, sizeof(LimLds), (hipStream_t)stream, x, ctl, y, gain, winner, N, nt, C, lookahead,
                           sample_rate, (float)eps);
    else
        hipLaunchKernelGGL(limiter_forward_kernel<false>, grid, block, sizeof(LimLds), (hipStream_t)stream, x, ctl, y, gain, winner, N, nt, C, lookahead,
                           sample_rate, (float)eps);
    return launch_status();
}

int dasp_limiter_backward(const float* x, const float* ctl, const float* gain, const int* winner, const float* gy, float* gx, float* gctl,
                          float* scratch, int B, int C, long N, int lookahead, double sample_rate, double eps, void* stream) {
    if (!gain || !winner || !gy || !gctl || !scratch) return DASP_ERR_ARG;
    int s = lim_args(x, ctl, B, C, N, lookahead, sample_rate, eps);
    if (s != DASP_OK) return s;
    if ((s = lim_prepare()) != DASP_OK) return s;
    const hipStream_t st = (hipStream_t)stream;
    if (zero_async(scratch, (size_t)B * N * 2 * sizeof(float), st) != hipSuccess) return launch_status();
    hipLaunchKernelGGL(limiter_backward_kernel, dim3((unsigned)B), dim3(LIM_THREADS), sizeof(LimLds), st, x, ctl, gain, winner, gy, gx, gctl,
                       reinterpret_cast<f2*>(scratch), N, (int)lim_ntile(N, lookahead), C, lookahead, sample_rate, (float)eps);
    return launch_status();
}

}  // extern "C"
