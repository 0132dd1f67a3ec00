// Time-domain losses (auraloss.time 0.4.0: ESRLoss, DCLoss, LogCoshLoss, SNRLoss, SISDRLoss, SDSDRLoss, and the MSE term the reference's
// examples/virtual_analog.py adds to its STFT loss) on one fused moment pass. Per row of N samples, with d = p - t, every one of these
// losses is a function of six sums
//     Sd = sum d, St = sum t, Sdd = sum d^2, Stt = sum t^2, Sdt = sum d t, Slc = sum log(cosh(a d) + eps)
// and every gradient is a per-row linear combination of d[n], t[n], 1 and sinh(a d[n]) / (cosh(a d[n]) + eps):
//     forward   one read of both signals (8 B per sample) -> per-workgroup partial sums in a scratch array; a one-wave-per-row launch adds
//               them in a fixed order, writes the moments in fp64 and the weighted per-row loss; a one-workgroup launch adds the rows for
//               reduction = mean / sum. No atomics, no counters, nothing to zero: bit-identical run to run and plain kernel nodes in a graph.
//     backward  one elementwise pass (8 B read + 4 B written per sample and gradient); a prologue per workgroup derives the row's
//               coefficients from the saved moments in fp64.
// The moments are taken on d, never rebuilt from sum p^2, sum p t, sum t^2: a trained model has p ~ t and that expansion cancels.
// Rows are not 16-byte aligned in general (odd N; a view with a storage offset): each (row, segment) walks scalar head samples up to the
// first 16-byte boundary of ONE of its pointers, 16-byte vectors from there, and a scalar tail. The other pointers go through a vector
// type that claims 4-byte alignment only - global dwordx4 accesses need no more - and are 16-byte aligned whenever they share the phase
// (the same row offset from an aligned base: the usual case).
#include "common.hpp"

#include <math.h>

using namespace dasp;

namespace {

constexpr int TD_NT = 256;                 // threads per workgroup of the two passes
constexpr long TD_MIN_SEG = 4096;          // samples per workgroup at least: four 16-byte loads per thread and signal
constexpr long TD_FILL = 1024;             // workgroups that fill the chip: 256 CUs x 4 workgroups (16 waves per CU, 8 loads in flight per lane)
enum { TD_SD = 0, TD_ST, TD_SDD, TD_STT, TD_SDT, TD_SLC, TD_NM };
enum { TD_W_ESR = 0, TD_W_DC, TD_W_LC, TD_W_SNR, TD_W_SISDR, TD_W_SDSDR, TD_W_MSE, TD_NW };
enum { TD_NONE = 0, TD_MEAN = 1, TD_SUM = 2 };

struct TdParams {
    double w[TD_NW];
    double a, eps;
    int zero_mean;
};

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));       // 16 bytes at a 4-byte aligned address
__device__ __forceinline__ f4 ld4u(const f4u* p) {       // ld_stream for it (the template would deduce the 16-byte aligned type)
#if DASP_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// log(cosh z + eps) without overflow and without losing eps beside 1: with E = e^-|z| (through expm1),
//   |z| < 1    cosh z - 1 = (E - 1)^2 / (2 E)                 -> log1p((E - 1)^2 / (2 E) + eps)
//   otherwise  cosh z + eps = e^|z| / 2 (1 + E^2 + 2 eps E)   -> |z| - log 2 + log1p(E (E + 2 eps))
__device__ __forceinline__ float td_lc(float z, float eps) {
    const float az = fabsf(z), em = expm1f(-az), E = 1.f + em;
    const bool small = az < 1.f;
    const float arg = small ? em * em / (2.f * E) + eps : E * (E + 2.f * eps);
    return (small ? 0.f : az - 0.69314718f) + log1pf(arg);
}
// its derivative sinh z / (cosh z + eps) = sign(z) (1 - E^2) / (1 + E^2 + 2 eps E), 1 - E^2 = -m from expm1 (no cancellation at small z)
__device__ __forceinline__ float td_dlc(float z, float eps) {
    const float em = expm1f(-fabsf(z)), E = 1.f + em, m = em * (2.f + em);
    return copysignf(-m / (2.f + m + 2.f * eps * E), z);
}

// The weighted loss of one row from its moments, and (GRAD) its partial derivatives G[k] with respect to the six moments. fp64. A weight
// of exactly 0 skips its term: an inf / nan there (log of a non-positive ratio, an overflowed Slc) never meets a 0 *.
template <bool GRAD>
__device__ double td_row(const double* __restrict__ M, double n, const TdParams& q, double* G) {
    const double Sd = M[TD_SD], St = M[TD_ST], Sdd = M[TD_SDD], Stt = M[TD_STT], Sdt = M[TD_SDT], eps = q.eps;
    double loss = 0.0;
    if (GRAD)
        for (int k = 0; k < TD_NM; ++k) G[k] = 0.0;
    if (q.w[TD_W_ESR] != 0.0) {                         // sum (t - p)^2 / (sum t^2 + eps)
        const double w = q.w[TD_W_ESR], den = Stt + eps;
        loss += w * Sdd / den;
        if (GRAD) { G[TD_SDD] += w / den; G[TD_STT] -= w * Sdd / (den * den); }
    }
    if (q.w[TD_W_DC] != 0.0) {                          // mean(t - p)^2 / (mean(t^2) + eps)
        const double w = q.w[TD_W_DC], m = Sd / n, den = Stt / n + eps;
        loss += w * m * m / den;
        if (GRAD) { G[TD_SD] += w * 2.0 * m / (n * den); G[TD_STT] -= w * m * m / (den * den * n); }
    }
    if (q.w[TD_W_LC] != 0.0) {                          // mean(log(cosh(a (p - t)) + eps) / a)
        const double w = q.w[TD_W_LC] / (q.a * n);
        loss += w * M[TD_SLC];
        if (GRAD) G[TD_SLC] += w;
    }
    if (q.w[TD_W_MSE] != 0.0) {                         // mean (p - t)^2
        const double w = q.w[TD_W_MSE] / n;
        loss += w * Sdd;
        if (GRAD) G[TD_SDD] += w;
    }
    if (q.w[TD_W_SNR] != 0.0 || q.w[TD_W_SISDR] != 0.0 || q.w[TD_W_SDSDR] != 0.0) {
        // E = sum d'^2, T = sum t'^2, C = sum d' t' of the (zero-mean) signals; the residual of the scaled target is
        // sum (p' - alpha t')^2 = E + 2 beta C + beta^2 T with beta = 1 - alpha = (eps - C) / (T + eps)
        double E = Sdd, T = Stt, C = Sdt;
        if (q.zero_mean) {
            E = Sdd - Sd * Sd / n;                      // x < 0 ? 0 : x, not fmax: a NaN / inf - inf moment stays NaN (fmax would
            T = Stt - St * St / n;                      // hand back 0, and SNRLoss of a diverged prediction would read as perfect)
            E = E < 0.0 ? 0.0 : E;
            T = T < 0.0 ? 0.0 : T;
            C = Sdt - Sd * St / n;
        }
        const double K = -4.342944819032518;            // -10 / ln 10
        double gE = 0.0, gT = 0.0, gC = 0.0;
        if (q.w[TD_W_SNR] != 0.0) {                     // -10 log10(T / (E + eps) + eps)
            const double w = q.w[TD_W_SNR], den = E + eps, ratio = T / den;
            loss += w * K * log(ratio + eps);
            if (GRAD) {
                const double dl = w * K / (ratio + eps);
                gT += dl / den;
                gE -= dl * ratio / den;
            }
        }
        const double Te = T + eps, alpha = (C + T) / Te, beta = (eps - C) / Te;
        if (q.w[TD_W_SISDR] != 0.0) {                   // -10 log10(alpha^2 T / (sum (p' - alpha t')^2 + eps) + eps)
            const double w = q.w[TD_W_SISDR], num = alpha * alpha * T, den = E + 2.0 * beta * C + beta * beta * T + eps, ratio = num / den;
            loss += w * K * log(ratio + eps);
            if (GRAD) {
                const double dl = w * K / (ratio + eps), dnum = 1.0 / den, dres = -ratio / den;
                const double dalpha = dnum * 2.0 * alpha * T - dres * (2.0 * C + 2.0 * beta * T);
                gE += dl * dres;
                gC += dl * (dres * 2.0 * beta + dalpha / Te);
                gT += dl * (dnum * alpha * alpha + dres * beta * beta + dalpha * beta / Te);
            }
        }
        if (q.w[TD_W_SDSDR] != 0.0) {                   // -10 log10(alpha^2 T / (E + eps) + eps)
            const double w = q.w[TD_W_SDSDR], den = E + eps, ratio = alpha * alpha * T / den;
            loss += w * K * log(ratio + eps);
            if (GRAD) {
                const double dl = w * K / (ratio + eps), dalpha = 2.0 * alpha * T / den;
                gE -= dl * ratio / den;
                gC += dl * dalpha / Te;
                gT += dl * (alpha * alpha / den + dalpha * beta / Te);
            }
        }
        if (GRAD) {
            G[TD_SDD] += gE; G[TD_STT] += gT; G[TD_SDT] += gC;
            if (q.zero_mean) {
                G[TD_SD] -= (2.0 * gE * Sd + gC * St) / n;
                G[TD_ST] -= (2.0 * gT * St + gC * Sd) / n;
            }
        }
    }
    return loss;
}

// samples [s0, s0 + len) of row r belong to workgroup r G + g; `anchor` is the pointer whose 16-byte boundaries the walk follows
struct TdSpan {
    long off, len, head, nvec, tail0;
};
__device__ __forceinline__ TdSpan td_span(const float* anchor, long N, long S, long G) {
    TdSpan s;
    const long r = (long)blockIdx.x / G, g = (long)blockIdx.x - r * G;
    const long s0 = g * S;
    s.off = r * N + s0;
    s.len = N - s0 < S ? N - s0 : S;
    s.head = (long)((4u - (unsigned)(((uintptr_t)(anchor + s.off) >> 2) & 3u)) & 3u);
    if (s.head > s.len) s.head = s.len;
    s.nvec = (s.len - s.head) >> 2;
    s.tail0 = s.head + 4 * s.nvec;
    return s;
}

struct TdAcc {
    float sd, st, sdd, stt, sdt, slc;
};
template <bool LC> __device__ __forceinline__ void td_add(TdAcc& A, float p, float t, float a, float eps) {
    const float d = p - t;
    A.sd += d;
    A.st += t;
    A.sdd = fmaf(d, d, A.sdd);
    A.stt = fmaf(t, t, A.stt);
    A.sdt = fmaf(d, t, A.sdt);
    if (LC) A.slc += td_lc(a * d, eps);
}
template <bool LC> __device__ __forceinline__ void td_add4(TdAcc& A, f4 p, f4 t, float a, float eps) {
    td_add<LC>(A, p.x, t.x, a, eps);
    td_add<LC>(A, p.y, t.y, a, eps);
    td_add<LC>(A, p.z, t.z, a, eps);
    td_add<LC>(A, p.w, t.w, a, eps);
}
__device__ __forceinline__ void td_flush(double (&D)[TD_NM], TdAcc& A) {     // the fp32 sums of at most 16 samples go into the fp64 ones
    D[TD_SD] += (double)A.sd; D[TD_ST] += (double)A.st; D[TD_SDD] += (double)A.sdd;
    D[TD_STT] += (double)A.stt; D[TD_SDT] += (double)A.sdt; D[TD_SLC] += (double)A.slc;
    A = TdAcc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// partials[(r G + g) 6 + k]: the six sums of segment g of row r. LC = false (w_log_cosh = 0) leaves Slc at 0 and evaluates nothing.
template <bool LC>
__global__ void __launch_bounds__(TD_NT) tdloss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           double* __restrict__ partials, long N, long S, long G, float a, float eps) {
    __shared__ double red[TD_NT / 64][TD_NM];
    const TdSpan s = td_span(pred, N, S, G);
    const float* __restrict__ p = pred + s.off;
    const float* __restrict__ t = target + s.off;
    const int tid = threadIdx.x;
    double D[TD_NM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    TdAcc A = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (tid < s.head) td_add<LC>(A, p[tid], t[tid], a, eps);
    if (s.tail0 + tid < s.len) td_add<LC>(A, p[s.tail0 + tid], t[s.tail0 + tid], a, eps);
    const f4* __restrict__ pv = reinterpret_cast<const f4*>(p + s.head);
    const f4u* __restrict__ tv = reinterpret_cast<const f4u*>(t + s.head);
    long v = tid;
    for (; v + 3 * TD_NT < s.nvec; v += 4 * TD_NT) {            // eight 16-byte loads in flight per lane
        f4 P[4], T[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            P[u] = ld_stream(pv + v + u * TD_NT);
            T[u] = ld4u(tv + v + u * TD_NT);
        }
        td_flush(D, A);
#pragma unroll
        for (int u = 0; u < 4; ++u) td_add4<LC>(A, P[u], T[u], a, eps);
    }
    for (; v < s.nvec; v += TD_NT) {                            // at most three more vectors
        const f4 P = ld_stream(pv + v), T = ld4u(tv + v);
        td_flush(D, A);
        td_add4<LC>(A, P, T, a, eps);
    }
    td_flush(D, A);
#pragma unroll
    for (int k = 0; k < TD_NM; ++k) D[k] = wave_sum(D[k]);
    if (lane_id() == 0)
        for (int k = 0; k < TD_NM; ++k) red[wave_id()][k] = D[k];
    __syncthreads();
    if (tid < TD_NM) {
        double acc = red[0][tid];
        for (int w = 1; w < TD_NT / 64; ++w) acc += red[w][tid];
        partials[(long)blockIdx.x * TD_NM + tid] = acc;
    }
}

// One wave per row: the row's G partials in a fixed order -> moments (fp64), the weighted loss of the row (fp32 out, fp64 for the scalar).
__global__ void __launch_bounds__(64) tdloss_rows_kernel(const double* __restrict__ partials, double* __restrict__ moments,
                                                         double* __restrict__ row_f64, float* __restrict__ row_loss, long N, long G, TdParams q) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    double m[TD_NM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long g = lane; g < G; g += 64)
        for (int k = 0; k < TD_NM; ++k) m[k] += partials[(r * G + g) * TD_NM + k];
#pragma unroll
    for (int k = 0; k < TD_NM; ++k) m[k] = wave_sum(m[k]);
    if (lane == 0) {
        for (int k = 0; k < TD_NM; ++k) moments[r * TD_NM + k] = m[k];
        const double loss = td_row<false>(m, (double)N, q, nullptr);
        row_f64[r] = loss;
        row_loss[r] = (float)loss;
    }
}

// reduction = mean / sum: the rows' losses in a fixed order
__global__ void __launch_bounds__(1024) tdloss_scalar_kernel(const double* __restrict__ row_f64, float* __restrict__ loss, long rows, double scale) {
    __shared__ double red[16];
    double acc = 0.0;
    for (long r = threadIdx.x; r < rows; r += 1024) acc += row_f64[r];
    acc = wave_sum(acc);
    if (lane_id() == 0) red[wave_id()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = red[0];
        for (int w = 1; w < 16; ++w) tot += red[w];
        *loss = (float)(tot * scale);
    }
}

// gpred[n] = c[0] + c[1] d[n] + c[2] t[n] + c[3] sinh(z) / (cosh(z) + eps), z = a d[n]; gtarget likewise with c[4..7]. Either may be NULL.
template <bool LC> __device__ __forceinline__ void td_grad(float p, float t, const float* c, float a, float eps, float& gp, float& gt) {
    const float d = p - t;
    gp = fmaf(c[1], d, fmaf(c[2], t, c[0]));
    gt = fmaf(c[5], d, fmaf(c[6], t, c[4]));
    if (LC) {
        const float sh = td_dlc(a * d, eps);
        gp = fmaf(c[3], sh, gp);
        gt = fmaf(c[7], sh, gt);
    }
}
template <bool LC> __device__ __forceinline__ void td_grad4(f4 p, f4 t, const float* c, float a, float eps, f4& gp, f4& gt) {
    float g0[4], g1[4];
    td_grad<LC>(p.x, t.x, c, a, eps, g0[0], g1[0]);
    td_grad<LC>(p.y, t.y, c, a, eps, g0[1], g1[1]);
    td_grad<LC>(p.z, t.z, c, a, eps, g0[2], g1[2]);
    td_grad<LC>(p.w, t.w, c, a, eps, g0[3], g1[3]);
    gp = f4{g0[0], g0[1], g0[2], g0[3]};
    gt = f4{g1[0], g1[1], g1[2], g1[3]};
}
template <bool LC>
__global__ void __launch_bounds__(TD_NT) tdloss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const double* __restrict__ moments, const float* __restrict__ gloss,
                                                           float* __restrict__ gpred, float* __restrict__ gtarget, long rows, long N, long S,
                                                           long G, TdParams q, int reduction) {
    __shared__ float cs[8];
    const int tid = threadIdx.x;
    if (tid == 0) {
        const long r = (long)blockIdx.x / G;
        double Gm[TD_NM];
        td_row<true>(moments + r * TD_NM, (double)N, q, Gm);
        double up = (double)(reduction == TD_NONE ? gloss[r] : gloss[0]);
        if (reduction == TD_MEAN) up /= (double)rows;
        const double lc = q.a * Gm[TD_SLC];
        // d F / d p = dF/dd; d F / d t = dF/dt - dF/dd for F(d, t) = loss(t + d, t)
        cs[0] = (float)(up * Gm[TD_SD]);
        cs[1] = (float)(up * 2.0 * Gm[TD_SDD]);
        cs[2] = (float)(up * Gm[TD_SDT]);
        cs[3] = (float)(up * lc);
        cs[4] = (float)(up * (Gm[TD_ST] - Gm[TD_SD]));
        cs[5] = (float)(up * (Gm[TD_SDT] - 2.0 * Gm[TD_SDD]));
        cs[6] = (float)(up * (2.0 * Gm[TD_STT] - Gm[TD_SDT]));
        cs[7] = (float)(-up * lc);
    }
    __syncthreads();
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = cs[k];
    const float a = (float)q.a, eps = (float)q.eps;
    const TdSpan s = td_span(gpred ? gpred : gtarget, N, S, G);        // the walk follows the stores of the first gradient
    const float* __restrict__ p = pred + s.off;
    const float* __restrict__ t = target + s.off;
    float* __restrict__ gp = gpred ? gpred + s.off : nullptr;
    float* __restrict__ gt = gtarget ? gtarget + s.off : nullptr;
    if (tid < 8) {                                                       // threads 0..3: head samples, 4..7: tail samples
        const long i = tid < 4 ? (long)tid : s.tail0 + (tid - 4);
        if (tid < 4 ? i < s.head : i < s.len) {
            float a0, a1;
            td_grad<LC>(p[i], t[i], c, a, eps, a0, a1);
            if (gp) gp[i] = a0;
            if (gt) gt[i] = a1;
        }
    }
    const f4u* __restrict__ pv = reinterpret_cast<const f4u*>(p + s.head);
    const f4u* __restrict__ tv = reinterpret_cast<const f4u*>(t + s.head);
    f4u* __restrict__ gpv = reinterpret_cast<f4u*>(gp ? gp + s.head : nullptr);
    f4u* __restrict__ gtv = reinterpret_cast<f4u*>(gt ? gt + s.head : nullptr);
    long v = tid;
    for (; v + 3 * TD_NT < s.nvec; v += 4 * TD_NT) {
        f4 P[4], T[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            P[u] = ld4u(pv + v + u * TD_NT);
            T[u] = ld4u(tv + v + u * TD_NT);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f4 A, B;
            td_grad4<LC>(P[u], T[u], c, a, eps, A, B);
            if (gpv) gpv[v + u * TD_NT] = A;
            if (gtv) gtv[v + u * TD_NT] = B;
        }
    }
    for (; v < s.nvec; v += TD_NT) {
        const f4 P = ld4u(pv + v), T = ld4u(tv + v);
        f4 A, B;
        td_grad4<LC>(P, T, c, a, eps, A, B);
        if (gpv) gpv[v] = A;
        if (gtv) gtv[v] = B;
    }
}

// Work split: a row is cut into segments of S samples (a multiple of 1024, at least TD_MIN_SEG) so that rows x segments reaches TD_FILL
// workgroups where the signal is long enough: 32 x 131072 -> 32 segments of 4096 per row (1024 workgroups), 512 x 131072 -> 2 segments of
// 65536 (1024 workgroups), 1024 rows and more -> one workgroup per row. The plan depends on (rows, N) alone: the forward, its size query
// and the backward agree without a device.
bool td_plan(long rows, long N, long* S, long* G) {
    if (rows < 1 || N < 1 || rows > (1L << 40) || N > (1L << 40) || rows > (1L << 60) / N) return false;
    const long want = (TD_FILL + rows - 1) / rows;
    long s = (N + want - 1) / want;
    if (s < TD_MIN_SEG) s = TD_MIN_SEG;
    s = (s + 1023) / 1024 * 1024;
    *S = s;
    *G = (N + s - 1) / s;
    return rows <= 0x7fffffffL / *G;             // one workgroup per (row, segment) on a one-dimensional grid
}

bool td_params(TdParams* q, const double* w, double a, double eps, int zero_mean) {
    bool any = false;
    for (int k = 0; k < TD_NW; ++k) {
        if (!isfinite(w[k])) return false;
        any = any || w[k] != 0.0;
        q->w[k] = w[k];
    }
    if (!any || !isfinite(a) || !(a > 0.0) || !isfinite(eps)) return false;
    q->a = a;
    q->eps = eps;
    q->zero_mean = zero_mean != 0;
    return true;
}

int td_check() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DASP_OK : (int)e;
}

}  // namespace

extern "C" {

long dasp_tdloss_scratch_doubles(long rows, long N) {
    long S, G;
    if (!td_plan(rows, N, &S, &G)) return -1;
    return rows * G * TD_NM + rows;
}

int dasp_tdloss_forward(const float* pred, const float* target, double* scratch, double* moments, float* row_loss, float* loss, long rows,
                        long N, double w_esr, double w_dc, double w_log_cosh, double w_snr, double w_si_sdr, double w_sd_sdr, double w_mse,
                        double a, double eps, int zero_mean, int reduction, void* stream) {
    const double w[TD_NW] = {w_esr, w_dc, w_log_cosh, w_snr, w_si_sdr, w_sd_sdr, w_mse};
    TdParams q;
    if (!pred || !target || !scratch || !moments || !row_loss || rows < 1 || N < 1 || reduction < TD_NONE || reduction > TD_SUM ||
        (reduction != TD_NONE && !loss) || !td_params(&q, w, a, eps, zero_mean))
        return DASP_ERR_ARG;
    long S, G;
    if (!td_plan(rows, N, &S, &G)) return DASP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    double* row_f64 = scratch + rows * G * TD_NM;
    const dim3 grid((unsigned)(rows * G));
    if (w_log_cosh != 0.0)
        hipLaunchKernelGGL(tdloss_fwd_kernel<true>, grid, dim3(TD_NT), 0, st, pred, target, scratch, N, S, G, (float)a, (float)eps);
    else
        hipLaunchKernelGGL(tdloss_fwd_kernel<false>, grid, dim3(TD_NT), 0, st, pred, target, scratch, N, S, G, (float)a, (float)eps);
    hipLaunchKernelGGL(tdloss_rows_kernel, dim3((unsigned)rows), dim3(64), 0, st, (const double*)scratch, moments, row_f64, row_loss, N, G, q);
    if (reduction != TD_NONE)
        hipLaunchKernelGGL(tdloss_scalar_kernel, dim3(1), dim3(1024), 0, st, (const double*)row_f64, loss, rows,
                           reduction == TD_MEAN ? 1.0 / (double)rows : 1.0);
    return td_check();
}

int dasp_tdloss_backward(const float* pred, const float* target, const double* moments, const float* gloss, float* gpred, float* gtarget,
                         long rows, long N, double w_esr, double w_dc, double w_log_cosh, double w_snr, double w_si_sdr, double w_sd_sdr,
                         double w_mse, double a, double eps, int zero_mean, int reduction, void* stream) {
    const double w[TD_NW] = {w_esr, w_dc, w_log_cosh, w_snr, w_si_sdr, w_sd_sdr, w_mse};
    TdParams q;
    if (!pred || !target || !moments || !gloss || (!gpred && !gtarget) || rows < 1 || N < 1 || reduction < TD_NONE || reduction > TD_SUM ||
        !td_params(&q, w, a, eps, zero_mean))
        return DASP_ERR_ARG;
    long S, G;
    if (!td_plan(rows, N, &S, &G)) return DASP_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(rows * G));
    if (w_log_cosh != 0.0)
        hipLaunchKernelGGL(tdloss_bwd_kernel<true>, grid, dim3(TD_NT), 0, (hipStream_t)stream, pred, target, moments, gloss, gpred, gtarget, rows,
                           N, S, G, q, reduction);
    else
        hipLaunchKernelGGL(tdloss_bwd_kernel<false>, grid, dim3(TD_NT), 0, (hipStream_t)stream, pred, target, moments, gloss, gpred, gtarget, rows,
                           N, S, G, q, reduction);
    return td_check();
}

}  // extern "C"
