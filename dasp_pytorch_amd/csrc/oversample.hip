// oversampled_distortion: tanh(g x) at L times the sample rate, fused - polyphase windowed-sinc interpolation by L, the non-linearity,
// low-pass and decimation by L in one kernel per direction. The L-times-longer signal lives in LDS only: forward 8 B of HBM traffic per
// base sample (read x, write y), backward 12 B (read x and gy, write gx; u is recomputed). Bound by vector-instruction issue, not HBM.
//
//   h[c], c = -H L .. H L: the symmetric taps (host, fp64, rounded once), here as hp[k] = h[k - H L], zero for k > 2 H L
//   u[L q + p] = sum_{d = 0 .. 2H} hp[d L + p] x[q + H - d]                      (x zero outside [0, N))
//   v[m]       = tanh(g u[m]) for 0 <= m < L N, zero outside;  g = 10^(drive_db / 20)
//   y[n]       = (1 / L) sum_p sum_{k = 0 .. 2H} hp[k L + p] v[L (n - H + k) + p]                     (T, and so every t0, is even)
// Adjoint, with the same two loops (h is symmetric):
//   w[L q + p] = (1 / L) sum_d hp[d L + p] gy[q + H - d],  s[m] = w[m] sech^2(g u[m]) inside [0, L N), zero outside
//   gx[j]      = g sum_p sum_k hp[k L + p] s[L (j - H + k) + p],   gdrive = ln10/20 g sum_m s[m] u[m]
//
// A workgroup owns T = OS_SLOTS / L - 2 OS_HMAX base samples of one (b, c) row, from t0 on. It stages x (and gy) over [t0 - 2H, t0 + T + 2H)
// in LDS, forms v (or s) for the base positions q in [t0 - H, t0 + T + H) - at most OS_SLOTS / L of them, so that the 256 threads
// take them in whole passes - and decimates from LDS. v is kept phase-major, plane p holding v[L q + p] at q - (t0 - H): the interpolator
// writes and the decimator reads one plane at consecutive words across the lanes of a wave (unit stride, no bank conflict; interleaved,
// the decimator would read at a stride of L words: L-way conflicts). The taps are a kernel argument: their index is wave-uniform, so
// they are read through the scalar cache and enter the fmas as scalar operands.
// The backward kernel writes one partial of sum s u per (row, tile) over the q the tile owns, [t0, t0 + T): every m is counted once; a
// finalize kernel adds them in fp64. No atomics, no waiting between workgroups: results are bit-identical run to run, and a row gives the
// same bits alone and inside a batch.
#include "row_helpers.hpp"

namespace dasp {

constexpr int OS_THREADS = 256;
constexpr int OS_HMAX = 16;                  // half width of the taps in base samples
constexpr int OS_LMAX = 8;
constexpr int OS_SLOTS = 4096;               // oversampled samples per workgroup in LDS (16 KiB), halo included
constexpr int OS_TAP_ROWS = 2 * OS_HMAX + 3;
struct OsTaps { float h[OS_TAP_ROWS * OS_LMAX]; };          // h[(k + 1) L + p] = hp[k L + p]: a row of zeros in front, zeros past 2 H L (padding that no loop multiplies)

// sech^2 in the form of elementwise.hip, 4 e / (1 + e)^2 with e = exp(-2 |u|): keeps its relative accuracy where tanh saturates. On the
// hardware exponential and reciprocal (1 ulp each; the argument's rounding costs e a relative 1e-6 only where e < 1e-10): this kernel is
// bound by vector-instruction issue, and expf with a true division is three times the instructions (backward call 0.913 -> 0.835 ms at
// (256,2,131072), 4x). A branch-free tanh on the same two instructions was measured too: forward 0.632 -> 0.597 ms, not worth a second
// tanh in the library - the forward pass keeps tanhf, as distortion does.
__device__ __forceinline__ float os_sech2(float u) {
    const float e = __expf(-2.f * fabsf(u)), r = __builtin_amdgcn_rcpf(1.f + e);
    return 4.f * e * r * r;
}

template <int L> struct OsTile {
    static constexpr int TQ = OS_SLOTS / L;              // base positions with a value in LDS
    static constexpr int T = TQ - 2 * OS_HMAX;           // base samples a workgroup owns
    static constexpr int XS = TQ + 2 * OS_HMAX;          // staged input samples (T + 4 H at most)
};

template <int L, bool BWD>
__global__ void __launch_bounds__(OS_THREADS)
osdist_kernel(const float* __restrict__ x, const float* __restrict__ drive_db, const OsTaps taps, const float* __restrict__ gy,
              float* __restrict__ out, float* __restrict__ partials, long N, int ntile, int H) {
    constexpr int TQ = OsTile<L>::TQ, T = OsTile<L>::T, XS = OsTile<L>::XS;
    __shared__ float xs[XS];
    __shared__ float gs[BWD ? XS : 1];
    __shared__ __attribute__((aligned(16))) float vs[L * TQ];      // plane p: v (forward) or s (backward) at [p * TQ + q - (t0 - H)]
    const int row = blockIdx.x / ntile, tile = blockIdx.x % ntile, tid = threadIdx.x;
    const long t0 = (long)tile * T;
    const float g = exp10f(drive_db[row] * 0.05f);
    const float* xr = x + (size_t)row * N;
    const float* gr = BWD ? gy + (size_t)row * N : nullptr;
    const int nx = T + 4 * H, nq = T + 2 * H, nk = 2 * H + 1;

    for (int i = tid; i < nx; i += OS_THREADS) {
        const long j = t0 - 2 * H + i;
        const bool in = j >= 0 && j < N;
        xs[i] = in ? xr[j] : 0.f;
        if (BWD) gs[i] = in ? gr[j] : 0.f;
    }
    __syncthreads();

    float part = 0.f;
    for (int qi = tid; qi < nq; qi += OS_THREADS) {
        const long q = t0 - H + qi;
        float u[L], w[L];
#pragma unroll
        for (int p = 0; p < L; ++p) u[p] = w[p] = 0.f;
        if (q >= 0 && q < N) {
            for (int d = 0; d < nk - 1; ++d) {
                const float xv = xs[qi + 2 * H - d];
                const float gv = BWD ? gs[qi + 2 * H - d] : 0.f;
#pragma unroll
                for (int p = 0; p < L; ++p) {
                    const float hv = taps.h[(d + 1) * L + p];
                    u[p] = __builtin_fmaf(hv, xv, u[p]);
                    if (BWD) w[p] = __builtin_fmaf(hv, gv, w[p]);
                }
            }
            // d = 2 H: phase 0 alone has a tap there (hp[2 H L]); the padded zeros of the other phases are not multiplied, 0 x inf is NaN
            u[0] = __builtin_fmaf(taps.h[nk * L], xs[qi], u[0]);
            if (BWD) w[0] = __builtin_fmaf(taps.h[nk * L], gs[qi], w[0]);
            const bool own = qi >= H && qi < H + T;
#pragma unroll
            for (int p = 0; p < L; ++p) {
                if (BWD) {
                    const float s = w[p] * (1.f / L) * os_sech2(g * u[p]);
                    if (own) part = __builtin_fmaf(s, u[p], part);
                    u[p] = s;
                } else {
                    u[p] = tanhf(g * u[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < L; ++p) vs[p * TQ + qi] = u[p];
    }
    __syncthreads();

    // decimation, two neighbouring outputs per thread: the words ni + 2 e and ni + 2 e + 1 of a plane (one 8-byte LDS read) carry taps
    // 2 e and 2 e + 1 of output ni and taps 2 e - 1 and 2 e of output ni + 1 - a quarter of the LDS instructions of one word per read
    float* orow = out + (size_t)row * N;
    for (int ni = 2 * tid; ni < T; ni += 2 * OS_THREADS) {
        const long n = t0 + ni;
        if (n >= N) break;
        float a0[L], a1[L];
#pragma unroll
        for (int p = 0; p < L; ++p) a0[p] = a1[p] = 0.f;
        // the first and the last pair are peeled: tap -1 (e = 0, output ni + 1), tap 2 H + 1 (e = H, output ni) and, for the phases
        // p > 0, tap 2 H are padded zeros, and a NaN or inf word under them belongs to a neighbouring output's footprint, not to these
#pragma unroll
        for (int p = 0; p < L; ++p) {
            const f2 v = *reinterpret_cast<const f2*>(&vs[p * TQ + ni]);
            const float h0 = taps.h[L + p], hp = taps.h[2 * L + p];
            a0[p] = __builtin_fmaf(hp, v.y, __builtin_fmaf(h0, v.x, a0[p]));
            a1[p] = __builtin_fmaf(h0, v.y, a1[p]);
        }
        for (int e = 1; e < H; ++e) {
#pragma unroll
            for (int p = 0; p < L; ++p) {
                const f2 v = *reinterpret_cast<const f2*>(&vs[p * TQ + ni + 2 * e]);
                const float hm = taps.h[2 * e * L + p], h0 = taps.h[(2 * e + 1) * L + p], hp = taps.h[(2 * e + 2) * L + p];
                a0[p] = __builtin_fmaf(hp, v.y, __builtin_fmaf(h0, v.x, a0[p]));
                a1[p] = __builtin_fmaf(h0, v.y, __builtin_fmaf(hm, v.x, a1[p]));
            }
        }
#pragma unroll
        for (int p = 0; p < L; ++p) {
            const f2 v = *reinterpret_cast<const f2*>(&vs[p * TQ + ni + 2 * H]);
            a1[p] = __builtin_fmaf(taps.h[2 * H * L + p], v.x, a1[p]);
            if (p == 0) {
                a0[0] = __builtin_fmaf(taps.h[(2 * H + 1) * L], v.x, a0[0]);
                a1[0] = __builtin_fmaf(taps.h[(2 * H + 1) * L], v.y, a1[0]);
            }
        }
        float s0 = a0[0], s1 = a1[0];
#pragma unroll
        for (int p = 1; p < L; ++p) { s0 += a0[p]; s1 += a1[p]; }
        const float scale = BWD ? g : 1.f / L;
        orow[n] = s0 * scale;
        if (n + 1 < N) orow[n + 1] = s1 * scale;
    }

    if (BWD) {
        __shared__ float red[OS_THREADS / 64];
        const float ws = wave_sum(part);
        if (lane_id() == 0) red[wave_id()] = ws;
        __syncthreads();
        if (tid == 0) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < OS_THREADS / 64; ++i) s += red[i];
            partials[(size_t)row * ntile + tile] = s;
        }
    }
}

// gdrive[row] = ln10/20 g sum over the row's tiles of partials, in fp64 and in tile order
__global__ void osdist_finalize_kernel(const float* __restrict__ partials, const float* __restrict__ drive_db, float* __restrict__ gdrive, long rows,
                                       int ntile) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double s = 0.0;
    const float* p = partials + (size_t)i * ntile;
    for (int k = 0; k < ntile; ++k) s += (double)p[k];
    gdrive[i] = (float)(s * 0.11512925464970228 * pow(10.0, (double)drive_db[i] * 0.05));
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline bool os_factor_ok(int L) { return L == 2 || L == 4 || L == 8; }
inline int os_tile(int L) { return OS_SLOTS / L - 2 * OS_HMAX; }
inline long os_ntile(long N, int L) { return (N + os_tile(L) - 1) / os_tile(L); }
inline OsTaps os_taps(const float* taps, int L, int H) {
    OsTaps t;
    const int n = 2 * H * L + 1;
    for (int k = 0; k < OS_TAP_ROWS * OS_LMAX; ++k) t.h[k] = (k >= L && k - L < n) ? taps[k - L] : 0.f;
    return t;
}

template <bool BWD>
int os_launch(const float* x, const float* drive_db, const float* taps, const float* gy, float* out, float* gdrive, float* partials, int B, int C,
              long N, int L, int H, void* stream) {
    if (!x || !drive_db || !taps || !out || (BWD && (!gy || !gdrive || !partials)) || B <= 0 || C <= 0 || N <= 0 || !os_factor_ok(L) || H < 1 ||
        H > OS_HMAX)
        return DASP_ERR_ARG;
    const long rows = (long)B * C, nt = os_ntile(N, L);
    if (rows * nt > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    const OsTaps t = os_taps(taps, L, H);
    const dim3 grid((unsigned)(rows * nt)), block(OS_THREADS);
    const hipStream_t st = (hipStream_t)stream;
#define DASP_OS_LAUNCH(LL) hipLaunchKernelGGL((osdist_kernel<LL, BWD>), grid, block, 0, st, x, drive_db, t, gy, out, partials, N, (int)nt, H)
    if (L == 2) DASP_OS_LAUNCH(2); else if (L == 4) DASP_OS_LAUNCH(4); else DASP_OS_LAUNCH(8);
#undef DASP_OS_LAUNCH
    int s = launch_status();
    if (s != DASP_OK || !BWD) return s;
    hipLaunchKernelGGL(osdist_finalize_kernel, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, st, (const float*)partials, drive_db, gdrive, rows,
                       (int)nt);
    return launch_status();
}
}  // namespace

extern "C" {

int dasp_osdist_tile(int L) { return os_factor_ok(L) ? os_tile(L) : DASP_ERR_ARG; }
long dasp_osdist_partial_floats(long rows, long N, int L) { return rows <= 0 || N <= 0 || !os_factor_ok(L) ? DASP_ERR_ARG : rows * os_ntile(N, L); }

int dasp_osdist_forward(const float* x, const float* drive_db, const float* taps, float* y, int B, int C, long N, int L, int H, void* stream) {
    return os_launch<false>(x, drive_db, taps, nullptr, y, nullptr, nullptr, B, C, N, L, H, stream);
}
int dasp_osdist_backward(const float* x, const float* drive_db, const float* taps, const float* gy, float* gx, float* gdrive, float* partials,
                         int B, int C, long N, int L, int H, void* stream) {
    return os_launch<true>(x, drive_db, taps, gy, gx, gdrive, partials, B, C, N, L, H, stream);
}

}  // extern "C"
