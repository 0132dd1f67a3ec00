// resample: polyphase windowed-sinc sample-rate conversion by the reduced ratio o : n (torchaudio.functional.resample's published
// algorithm as DESIGN 3.15 states it), and its adjoint. With width = ceil(lowpass_filter_width o / base), base = min(o, n) rolloff:
//
//   forward   y[q n + r] = sum_k h[r][k] x[q o + k - width]           x zero outside [0, N),  j = q n + r < M = ceil(n N / o)
//   backward  gx[q o + s] = sum_j h[j mod n][q o + s + width - (j div n) o] gy[j]   over the j whose span covers the sample: a gather
//
// h[r][k] is zero by definition where the window's argument was clamped, so phase r has a compact span of cnt[r] consecutive taps, and
// the j that read one input sample are consecutive too: both directions have ONE form,
//
//   out[Q A + p] = sum_{m < cnt[p]} T[m][p] in[Q B + off[p] + m]       p in [0, A), `in` zero outside its row,
//
// forward with (A, B) = (n, o), off[r] = first[r] - width, T[m][r] = h[r][first[r] + m]; backward with (A, B) = (o, n), off[s] the first
// j (relative to Q n, it may be negative) and T the same float32 values transposed. Both tables are built on the host in float64
// (dasp_pytorch_amd/_resample_design.py) and live in device memory as A P + A words: the taps TAP-MAJOR, T[m A + p], P = max
// cnt, then one word per phase, (off[p] - lo) | cnt[p] << 16 with lo = min off.
//
// One workgroup owns F whole frames (F A consecutive outputs, dasp_resample_tile) of one row. It copies the table into LDS, stages the
// input window [Q0 B + lo, (Q0 + F - 1) B + lo + span) zero-filled outside the row (span = max (off + cnt) - lo; forward: at most
// F o + 2 width words), and thread t takes the outputs t, t + 256, ... of the tile: consecutive lanes hold consecutive phases, so the
// tap reads T[m A + p] fall on consecutive LDS banks whatever A is (no padding needed), the window reads lie B / A words apart from lane
// to lane (a broadcast or neighbouring banks when upsampling, up to ceil(B / A)-way bank conflicts when downsampling), and the stores
// are one lane per consecutive sample. Exactly cnt[p] products are formed per output, in ascending m, with float32 FMAs from zero: an
// output's sum depends on its phase only - bit-identical for a row alone or in a batch, for any N, run to run - and a NaN reaches only
// the outputs whose span covers it. No atomics, no scratch, nothing saved between the directions.
#include <atomic>

#include "row_helpers.hpp"

namespace dasp {

constexpr int RS_THREADS = 256;
constexpr int RS_TABLE_MAX = 16384;                  // taps of a table, A P
constexpr int RS_WINDOW_MAX = 20480;                 // words of the staged window
constexpr int RS_LDS_MAX = 40448;                    // table + phase words + window: 158 KiB of the workgroup's 160
// Developer A/B switches (tools/bench_resample.py --kernels against variant builds); DESIGN 3.15 "measured" has the numbers behind the defaults.
#ifndef DASP_RS_TILE
#define DASP_RS_TILE 2048          // outputs per workgroup where the window allows it
#endif
#ifndef DASP_RS_TABLE
#define DASP_RS_TABLE 0            // 0: taps in LDS tap-major, T[m A + p]; 1: in LDS phase-major with an odd row stride, T[p (P | 1) + m]; 2: read from
#endif                             // global memory tap-major (coalesced across lanes, served by the L1 / L2)
constexpr int RS_TILE_TARGET = DASP_RS_TILE;

__host__ __device__ __forceinline__ long rs_tab_words(int A, int P) {    // LDS words of the taps
    return DASP_RS_TABLE == 2 ? 0 : (long)A * (DASP_RS_TABLE == 1 ? (P | 1) : P);
}

// frames per workgroup; 0: the design does not fit
__host__ __device__ __forceinline__ int rs_frames(int A, int B, int P, int span) {
    if (A < 1 || B < 1 || P < 1 || span < P || (long)A * P > RS_TABLE_MAX || span > RS_WINDOW_MAX) return 0;
    const int want = RS_TILE_TARGET / A < 1 ? 1 : RS_TILE_TARGET / A;
    const int room = (RS_WINDOW_MAX - span) / B + 1;
    const int F = want < room ? want : room;
    return rs_tab_words(A, P) + A + (long)(F - 1) * B + span <= RS_LDS_MAX ? F : 0;
}
__host__ __device__ __forceinline__ int rs_window(int F, int B, int span) { return (F - 1) * B + span; }

__device__ __forceinline__ void rs_tile(const float* __restrict__ in, const unsigned* __restrict__ table, float* __restrict__ out, long len_in,
                                        long len_out, int A, int B, int P, int lo, int span, int F, unsigned tiles) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x, ntab = A * P, nlds = (int)rs_tab_words(A, P), wlen = rs_window(F, B, span);
    float* tab = rs_lds;                                                   // T[m A + p]
    unsigned* meta = reinterpret_cast<unsigned*>(rs_lds + nlds);           // (off - lo) | cnt << 16
    float* win = rs_lds + nlds + A;
    const unsigned row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const long Q0 = (long)tile * F;
    const float* inr = in + (size_t)row * len_in;
    float* outr = out + (size_t)row * len_out;

#if DASP_RS_TABLE == 0
    for (int i = tid; i < ntab; i += RS_THREADS) tab[i] = __builtin_bit_cast(float, table[i]);
#elif DASP_RS_TABLE == 1
    for (int i = tid; i < ntab; i += RS_THREADS) tab[(i % A) * (P | 1) + i / A] = __builtin_bit_cast(float, table[i]);
#endif
    for (int p = tid; p < A; p += RS_THREADS) {                            // held inside the window whatever the table says
        const unsigned w = table[ntab + p];
        const int cnt = min((int)(w >> 16), P), off = min((int)(w & 0xffffu), span - cnt);
        meta[p] = (unsigned)off | (unsigned)cnt << 16;
    }
    const long g0 = Q0 * B + lo;
    for (int i = tid; i < wlen; i += RS_THREADS) {
        const long g = g0 + i;
        win[i] = (g >= 0 && g < len_in) ? ld_stream(inr + g) : 0.f;
    }
    __syncthreads();

    const long j0 = Q0 * A;
    const int Tc = (int)min((long)F * A, len_out - j0);
    const int dq = RS_THREADS / A, dp = RS_THREADS - dq * A;
    int ql = tid / A, p = tid - ql * A;
    for (int jl = tid; jl < Tc; jl += RS_THREADS) {
        const unsigned w = meta[p];
        const int cnt = (int)(w >> 16);
        const float* x = win + ql * B + (int)(w & 0xffffu);
        float acc = 0.f;
        int m = 0;
        // four taps per trip (the products still enter the sum one by one, in ascending m), then the rest: cnt differs from lane to lane
#if DASP_RS_TABLE == 1
        const float* h = tab + p * (P | 1);
        for (; m + 4 <= cnt; m += 4) {
            acc = __builtin_fmaf(h[m], x[m], acc);
            acc = __builtin_fmaf(h[m + 1], x[m + 1], acc);
            acc = __builtin_fmaf(h[m + 2], x[m + 2], acc);
            acc = __builtin_fmaf(h[m + 3], x[m + 3], acc);
        }
        for (; m < cnt; ++m) acc = __builtin_fmaf(h[m], x[m], acc);
#else
        const float* h = (DASP_RS_TABLE == 0 ? tab : reinterpret_cast<const float*>(table)) + p;
        for (; m + 4 <= cnt; m += 4) {
            const float* hm = h + m * A;
            acc = __builtin_fmaf(hm[0], x[m], acc);
            acc = __builtin_fmaf(hm[A], x[m + 1], acc);
            acc = __builtin_fmaf(hm[2 * A], x[m + 2], acc);
            acc = __builtin_fmaf(hm[3 * A], x[m + 3], acc);
        }
        for (; m < cnt; ++m) acc = __builtin_fmaf(h[m * A], x[m], acc);
#endif
        st_stream(outr + j0 + jl, acc);
        p += dp; ql += dq;
        if (p >= A) { p -= A; ++ql; }
    }
}

__global__ void __launch_bounds__(RS_THREADS)
resample_forward_kernel(const float* __restrict__ x, const unsigned* __restrict__ table, float* __restrict__ y, long N, long M, int o, int n, int P,
                        int lo, int span, int F, unsigned tiles) {
    rs_tile(x, table, y, N, M, n, o, P, lo, span, F, tiles);
}

__global__ void __launch_bounds__(RS_THREADS)
resample_backward_kernel(const float* __restrict__ gy, const unsigned* __restrict__ table, float* __restrict__ gx, long N, long M, int o, int n,
                         int P, int lo, int span, int F, unsigned tiles) {
    rs_tile(gy, table, gx, M, N, o, n, P, lo, span, F, tiles);
}

constexpr int RS_FILL_WORDS = 960;                   // words of a table that one fill launch carries in its arguments
struct RsFill { unsigned w[RS_FILL_WORDS]; };
__global__ void __launch_bounds__(RS_THREADS) resample_fill_kernel(unsigned* __restrict__ dst, const RsFill f, int count) {
    for (int i = threadIdx.x; i < count; i += RS_THREADS) dst[i] = f.w[i];
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline size_t rs_lds_bytes(int A, int B, int P, int span, int F) { return ((size_t)rs_tab_words(A, P) + A + rs_window(F, B, span)) * sizeof(float); }

// The table and the window together are more LDS than a kernel gets unasked (64 KiB): asked for once per device - by
// dasp_resample_prepare() when the library is loaded, so that no call has to (a call may be under stream capture) - and by the first
// call on any other device.
int rs_prepare() {
    static std::atomic<bool> asked[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorNoDevice;
    if (dev >= 0 && dev < 64 && asked[dev].load(std::memory_order_acquire)) return DASP_OK;
    for (const void* f : {reinterpret_cast<const void*>(resample_forward_kernel), reinterpret_cast<const void*>(resample_backward_kernel)}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX * (int)sizeof(float));
        if (e != hipSuccess) return (int)e;
    }
    if (dev >= 0 && dev < 64) asked[dev].store(true, std::memory_order_release);
    return DASP_OK;
}

inline long rs_ceil_div(long a, long b) { return (a + b - 1) / b; }

// A, B: the periods of the output and the input of this direction. Returns the frames per workgroup (> 0) or a status.
int rs_args(const void* in, const void* table, const void* out, long rows, long N, long M, int o, int n, int A, int B, int P, int lo, int span,
            long len_out, unsigned* tiles) {
    if (!in || !table || !out || rows <= 0 || N <= 0 || M <= 0 || o <= 0 || n <= 0 || P <= 0 || span < P) return DASP_ERR_ARG;
    if (N > 0x7fffffffffffffffL / n || M != rs_ceil_div(n * N, (long)o)) return DASP_ERR_ARG;
    if (lo > B || lo < -RS_WINDOW_MAX) return DASP_ERR_ARG;
    const int F = rs_frames(A, B, P, span);
    if (F <= 0) return DASP_ERR_UNSUPPORTED;
    const long t = rs_ceil_div(len_out, (long)F * A);
    if (t > 0x7fffffffL || rows > 0x7fffffffL / t) return DASP_ERR_UNSUPPORTED;
    *tiles = (unsigned)t;
    return F;
}
}  // namespace

extern "C" {

int dasp_resample_table_limit(void) { return RS_TABLE_MAX; }
int dasp_resample_window_limit(void) { return RS_WINDOW_MAX; }
int dasp_resample_tile(int out_period, int in_period, int taps, int span) {
    if (out_period < 1 || in_period < 1 || taps < 1 || span < taps) return DASP_ERR_ARG;
    const int F = rs_frames(out_period, in_period, taps, span);
    return F > 0 ? F * out_period : DASP_ERR_UNSUPPORTED;
}
long dasp_resample_table_words(int out_period, int taps) {
    if (out_period < 1 || taps < 1) return DASP_ERR_ARG;
    return (long)out_period * taps <= RS_TABLE_MAX ? (long)out_period * taps + out_period : DASP_ERR_UNSUPPORTED;
}
int dasp_resample_prepare(void) { return rs_prepare(); }

int dasp_resample_table_store(void* dst, const void* host_words, long words, void* stream) {
    if (!dst || !host_words || words <= 0) return DASP_ERR_ARG;
    if (words > 2L * RS_TABLE_MAX) return DASP_ERR_UNSUPPORTED;
    const unsigned* src = static_cast<const unsigned*>(host_words);
    for (long at = 0; at < words; at += RS_FILL_WORDS) {
        const int count = (int)(words - at < RS_FILL_WORDS ? words - at : RS_FILL_WORDS);
        RsFill f = {};
        for (int i = 0; i < count; ++i) f.w[i] = src[at + i];
        hipLaunchKernelGGL(resample_fill_kernel, dim3(1), dim3(RS_THREADS), 0, (hipStream_t)stream, static_cast<unsigned*>(dst) + at, f, count);
        const int s = launch_status();
        if (s != DASP_OK) return s;
    }
    return DASP_OK;
}

int dasp_resample_forward(const float* x, const void* table, float* y, long rows, long N, long M, int orig, int new_, int taps, int lo, int span,
                          void* stream) {
    unsigned tiles = 0;
    const int F = rs_args(x, table, y, rows, N, M, orig, new_, new_, orig, taps, lo, span, M, &tiles);
    if (F <= 0) return F;
    int s = rs_prepare();
    if (s != DASP_OK) return s;
    hipLaunchKernelGGL(resample_forward_kernel, dim3((unsigned)(rows * tiles)), dim3(RS_THREADS), rs_lds_bytes(new_, orig, taps, span, F),
                       (hipStream_t)stream, x, static_cast<const unsigned*>(table), y, N, M, orig, new_, taps, lo, span, F, tiles);
    return launch_status();
}

int dasp_resample_backward(const float* gy, const void* table, float* gx, long rows, long N, long M, int orig, int new_, int taps, int lo, int span,
                           void* stream) {
    unsigned tiles = 0;
    const int F = rs_args(gy, table, gx, rows, N, M, orig, new_, orig, new_, taps, lo, span, N, &tiles);
    if (F <= 0) return F;
    int s = rs_prepare();
    if (s != DASP_OK) return s;
    hipLaunchKernelGGL(resample_backward_kernel, dim3((unsigned)(rows * tiles)), dim3(RS_THREADS), rs_lds_bytes(orig, new_, taps, span, F),
                       (hipStream_t)stream, gy, static_cast<const unsigned*>(table), gx, N, M, orig, new_, taps, lo, span, F, tiles);
    return launch_status();
}

}  // extern "C"
