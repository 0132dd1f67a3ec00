// Filtering by a supplied frequency response: y = irfft(rfft(x, n) * H, n), circular convolution of length n, not cropped.
//
// Replaces dasp_pytorch.signal.freqdomain_fir (dasp_pytorch/signal.py:35-39), forward and adjoint, on the library's own register/LDS
// transforms (fft_lds.hpp). x (rows, T) real, H (h_rows, n/2 + 1) complex in natural rfft order, rows = h_rows * chs: the chs
// consecutive rows of an item share one response (chs = 1: a response per row). n = 2^3 .. 2^20.
//
// Real input, complex transforms: two rows of an item travel as ONE complex frame x0 + i x1. The response is extended to all n bins
// as Hext[k] = H[k] (k <= n/2), conj(H[n - k]) (k > n/2), with the imaginary parts of bins 0 and n/2 dropped (irfft ignores them):
// Hext is Hermitian, so IFFT(FFT(x0 + i x1) Hext) = y0 + i y1 and no split is ever needed forward. An odd row left over (and every
// row when chs = 1) goes alone with a zero imaginary part.
//
// Adjoint. gx = first T samples of IFFT(FFT(gy) conj(Hext)) - the same kernels with the conjugate response. With Z = FFT(x0 + i x1)
// and G = FFT(gy0 + i gy1) of a frame, conj(X0) GY0 + conj(X1) GY1 = Herm(conj(Z) G), Herm(P)[k] = (P[k] + conj(P[n - k])) / 2
// (substitute the Hermitian splits of Z and G: the cross terms cancel), so
//     gH[k] = w_k / n * Herm(sum_frames conj(Z) G)[k],   w_k = 2 inside, 1 at bins 0 and n/2 (whose imaginary part is set to 0),
// PyTorch's convention for the gradient of a complex tensor. The frames of an item are summed in frame order by the one wave or
// workgroup that owns the item's bins: no atomics, bit-identical from run to run. X is recomputed from x; no spectrum is saved.
//
// n <= 8192: one launch per direction (fdfir_small_kernel): 8192 / n items side by side in a 1024-thread workgroup (col_fft), global
//     loads and stores staged through LDS so that side-by-side rows are still read and written as whole lines; the product with Hext
//     stays in registers between the two transforms. Nothing complex goes to memory.
// n >= 16384: four-step n = NA x 512 (time index ja * 512 + jb, frequency index ka + NA * kb), as the long convolution of reverb.hip:
//     fdfir_load_kernel   column transforms over ja of the zero-padded / cropped rows                  -> A[frame][ka][jb]
//     fdfir_rows_kernel   per row ka (one wave): twiddle, 512-point transform, product with Hext fetched in NATURAL bin order
//                         (k = ka + NA kb, mirrored and conjugated above n/2), inverse transform, conjugate twiddle; in place
//     fdfir_cols_kernel   inverse column transforms, scaled stores of the real (row 2f) and imaginary (row 2f + 1) parts
//     backward: the row pass also accumulates P = sum_frames conj(Z) G per item in the permuted order, and fdfir_gh_kernel takes its
//     Hermitian part into natural order (16 x 16 tiles of (ka, kb): 128-byte runs on the read and on the write side).
#include "common.hpp"
#include "fft_lds.hpp"

namespace dasp {

constexpr int FD_LOG = 13;                 // the single-launch workgroup: 1024 threads, 8192 elements
typedef ColGeom<FD_LOG> FdGeom;
typedef ColGeom<12> FdLoadGeom;            // column pass of the four-step transform, time -> A
constexpr int FD_NB = 512;                 // row length of the four-step split
constexpr int FD_MIN_LOG = 3, FD_MAX_LOG = 20;

struct FdDims {
    int logn, n, bins;       // transform length, n / 2 + 1
    int T;                   // samples per row of x (and of gx)
    int items, chs, nf;      // responses, rows per response, frames per response = (chs + 1) / 2
    int logNA, NA;           // four-step only
};

// Hext[k], k = 0 .. n - 1, from the n / 2 + 1 bins of one response
__device__ __forceinline__ f2 fd_hext(const f2* __restrict__ Hrow, int k, int n) {
    const int half = n >> 1, kk = k <= half ? k : n - k;
    f2 h = Hrow[kk];
    if (k > half) h.y = -h.y;
    if (kk == 0 || kk == half) h.y = 0.f;
    return h;
}

// ---- n <= 8192 --------------------------------------------------------------------------------------------------------------------
// Tile of TC items x P samples between global memory and the threads' registers, through LDS: the flat index e = t + P c walks rows
// contiguously (whole lines per wave), thread (j, c) owns t = j + T q. Row pitch P + 1 floats: both sides free of bank conflicts.
// Rows 2f (-> re) and 2f + 1 (-> im, zero when the item has no such row); samples t >= limit read as zero.
__device__ __forceinline__ void fd_stage_load(const float* __restrict__ src, int rowlen, int limit, const FdDims& d, const ColCfg& g, int item0, int f,
                                              float* sre, float* sim, float (&r)[8], float (&i)[8]) {
    const int pitch = g.P + 1;
    const bool has1 = 2 * f + 1 < d.chs;
    // the thread coordinates pass through an opaque move: otherwise every address of every staging step is computed once at the top of
    // the kernel and kept live across the transforms (128 registers per thread at 1024 threads)
    int tid = threadIdx.x, gj = g.j, gc = g.c;
    asm volatile("" : "+v"(tid), "+v"(gj), "+v"(gc));
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {           // two batches of 4 + 4 loads, each issued together at addresses that are always valid
        float v0[4], v1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + FdGeom::T * (4 * h + q), c = e >> d.logn, t = e & (g.P - 1);
            const int it = item0 + c < d.items ? item0 + c : d.items - 1, tc = t < limit ? t : limit - 1;
            const float* p = src + ((long)it * d.chs + 2 * f) * rowlen + tc;
            v0[q] = *p;
            v1[q] = p[has1 ? rowlen : 0];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + FdGeom::T * (4 * h + q), c = e >> d.logn, t = e & (g.P - 1);
            const bool ok = item0 + c < d.items && t < limit;
            sre[c * pitch + t] = ok ? v0[q] : 0.f;
            sim[c * pitch + t] = ok && has1 ? v1[q] : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) { r[q] = sre[gc * pitch + gj + g.T * q]; i[q] = sim[gc * pitch + gj + g.T * q]; }
}
__device__ __forceinline__ void fd_stage_store(float* __restrict__ dst, int rowlen, int limit, const FdDims& d, const ColCfg& g, int item0, int f,
                                               float* sre, float* sim, const float (&r)[8], const float (&i)[8]) {
    const int pitch = g.P + 1;
    const bool has1 = 2 * f + 1 < d.chs;
    // the thread coordinates pass through an opaque move: otherwise every address of every staging step is computed once at the top of
    // the kernel and kept live across the transforms (128 registers per thread at 1024 threads)
    int tid = threadIdx.x, gj = g.j, gc = g.c;
    asm volatile("" : "+v"(tid), "+v"(gj), "+v"(gc));
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) { sre[gc * pitch + gj + g.T * q] = r[q]; sim[gc * pitch + gj + g.T * q] = i[q]; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = tid + FdGeom::T * q, c = e >> d.logn, t = e & (g.P - 1);
        if (item0 + c < d.items && t < limit) {
            const long row = (long)(item0 + c) * d.chs + 2 * f;
            dst[row * rowlen + t] = sre[c * pitch + t];
            if (has1) dst[(row + 1) * rowlen + t] = sim[c * pitch + t];
        }
    }
}

// grid (ceil(items / TC), BWD ? 1 : nf). Thread (j, c): item blockIdx.x * TC + c, bins / samples j + (n / 8) q.
//   forward   out = y (rows, n)
//   backward  src = gy (rows, n); out = gx (rows, T) when want_out; gH (items, bins) when want_gh (the workgroup walks the item's frames)
template <bool BWD>
__global__ __launch_bounds__(FdGeom::T) void fdfir_small_kernel(const float* __restrict__ x, const f2* __restrict__ H, const float* __restrict__ gy,
                                                                const f2* __restrict__ tw, float* __restrict__ out, f2* __restrict__ gH, FdDims d,
                                                                int want_out, int want_gh) {
    __shared__ f2 lds[FdGeom::LDS];
    float* sre = reinterpret_cast<float*>(lds);
    float* sim = sre + FdGeom::LDS;
    const ColCfg g = col_config<FD_LOG>(d.logn, threadIdx.x);
    const int item0 = blockIdx.x * g.TC, item = item0 + g.c;
    const bool valid = item < d.items;
    const f2* Hrow = H + (long)(valid ? item : d.items - 1) * d.bins;
    const float inv = 1.f / (float)d.n;
    const int Tin = d.T < d.n ? d.T : d.n;                       // samples of a row of x that enter the transform (and of gx that leave it)
    const int f_lo = BWD ? 0 : (int)blockIdx.y, f_hi = BWD ? d.nf : f_lo + 1;
    // P = sum_f conj(Z) G lives in LDS, slot q * 1024 + thread: private to its thread until the Hermitian step (16 registers the loop
    // does not have to spare)
    __shared__ f2 pacc[BWD ? FdGeom::N : 1];
    if (BWD && want_gh) {
#pragma unroll
        for (int q = 0; q < 8; ++q) pacc[q * FdGeom::T + threadIdx.x] = f2{0.f, 0.f};
    }
    for (int f = f_lo; f < f_hi; ++f) {
        float r[8], i[8];
        if (BWD) fd_stage_load(gy, d.n, d.n, d, g, item0, f, sre, sim, r, i);
        else fd_stage_load(x, d.T, Tin, d, g, item0, f, sre, sim, r, i);
        col_fft<-1, FD_LOG>(r, i, g, tw, lds);
        if (BWD && want_gh) {
            float xr[8], xi[8];
            fd_stage_load(x, d.T, Tin, d, g, item0, f, sre, sim, xr, xi);
            col_fft<-1, FD_LOG>(xr, xi, g, tw, lds);
#pragma unroll
            for (int q = 0; q < 8; ++q) {          // P += conj(Z) G
                f2* a = pacc + (BWD ? q * FdGeom::T + threadIdx.x : 0);
                *a += f2{xr[q] * r[q] + xi[q] * i[q], xr[q] * i[q] - xi[q] * r[q]};
            }
        }
        if (!BWD || want_out) {
            f2 h[8];                                 // fetched here, not held across the transforms (128 registers per thread)
            int kj = g.j;
            asm volatile("" : "+v"(kj));
#pragma unroll
            for (int q = 0; q < 8; ++q) h[q] = fd_hext(Hrow, kj + g.T * q, d.n);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float hx = h[q].x * inv, hy = (BWD ? -h[q].y : h[q].y) * inv;
                const float t = r[q] * hx - i[q] * hy;
                i[q] = r[q] * hy + i[q] * hx;
                r[q] = t;
            }
            col_fft<1, FD_LOG>(r, i, g, tw, lds);
            if (BWD) fd_stage_store(out, d.T, Tin, d, g, item0, f, sre, sim, r, i);
            else fd_stage_store(out, d.n, d.n, d, g, item0, f, sre, sim, r, i);
        }
    }
    if (BWD && want_gh) {
        // Hermitian part of P: bin n - k of the same item, element j' + T q' of thread (j', c)
        __syncthreads();
        const int half = d.n >> 1, logT = d.logn - 3;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = g.j + g.T * q;
            if (valid && k <= half) {
                const int km = (d.n - k) & (d.n - 1);
                const f2 a = pacc[BWD ? q * FdGeom::T + threadIdx.x : 0];
                const f2 m = pacc[BWD ? (km >> logT) * FdGeom::T + (km & (g.T - 1)) * g.TC + g.c : 0];
                const bool edge = k == 0 || k == half;
                const float w = edge ? 0.5f * inv : inv;                  // w_k / n / 2
                gH[(long)item * d.bins + k] = f2{(a.x + m.x) * w, edge ? 0.f : (a.y - m.y) * w};
            }
        }
    }
}

// ---- n >= 16384: four-step -----------------------------------------------------------------------------------------------------------
// Column pass, time -> A[frame][ka][jb]. grid (n / 4096 column tiles, frames), 512 threads; thread (j, c): column jb = tile * TC + c,
// elements ja = j + (NA / 8) q. Rows 2f (real) and 2f + 1 (imaginary) of the frame's item, samples >= limit read as zero.
__global__ __launch_bounds__(FdLoadGeom::T) void fdfir_load_kernel(const float* __restrict__ src, const f2* __restrict__ tw, f2* __restrict__ A, FdDims d,
                                                                   int rowlen, int limit) {
    __shared__ f2 lds[FdLoadGeom::LDS];
    const ColCfg g = col_config<12>(d.logNA, threadIdx.x);
    const int frame = blockIdx.y, item = frame / d.nf, f = frame % d.nf;
    const bool has1 = 2 * f + 1 < d.chs;
    const long row = (long)item * d.chs + 2 * f;
    const int jb = xcd_tile(blockIdx.x, gridDim.x) * g.TC + g.c;
    float r[8], i[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {           // loads first at clamped addresses, the bounds applied to the values afterwards
        const int tt = (g.j + g.T * q) * FD_NB + jb, tc = tt < limit ? tt : limit - 1;
        r[q] = src[row * rowlen + tc];
        i[q] = has1 ? src[(row + 1) * rowlen + tc] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int tt = (g.j + g.T * q) * FD_NB + jb;
        r[q] = tt < limit ? r[q] : 0.f;
        i[q] = tt < limit ? i[q] : 0.f;
    }
    col_fft<-1>(r, i, g, tw, lds);
    f2* o = A + (long)frame * d.n;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[(long)(g.j + g.T * q) * FD_NB + jb] = f2{r[q], i[q]};
}

// Row pass, in place. grid (NA / 8, items), 512 threads = 8 waves, wave = row ka of the item's frames, lane j holds columns j + 64 q.
//   forward   A[f] = rowIFFT(rowFFT(A[f] tw) Hext) conj(tw) / n
//   backward  the same with conj(Hext) on the frames of gy (want_out), and P = sum_f conj(rowFFT(Ax[f] tw)) rowFFT(A[f] tw) (want_gh)
template <bool BWD>
__global__ __launch_bounds__(FFT_T, BWD ? 2 : 4) void fdfir_rows_kernel(f2* __restrict__ A, const f2* __restrict__ Ax, const f2* __restrict__ tw,
                                                                        const f2* __restrict__ H, f2* __restrict__ Pout, FdDims d, int want_out, int want_gh) {
    __shared__ f2 lds_all[FFT_T / 64][FFT512_LDS];
    const int j = lane_id(), v = wave_id();
    const int ka = blockIdx.x * (FFT_T / 64) + v, item = blockIdx.y;
    f2* lds = lds_all[v];
    const Fft512Tw t5 = fft512_twiddles(j, tw);
    float wr[8], wi[8];
    fourstep_twiddles(ka, j, d.n, wr, wi);
    const long rowoff = (long)ka * FD_NB + j;
    const f2* Hrow = H + (long)item * d.bins;
    const float inv = 1.f / (float)d.n;
    float hr[8], hi[8], pr[8], pi[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f2 h = fd_hext(Hrow, ka + d.NA * (j + 64 * q), d.n);
        hr[q] = h.x * inv; hi[q] = (BWD ? -h.y : h.y) * inv;
        pr[q] = 0.f; pi[q] = 0.f;
    }
    auto load_spec = [&](const f2* base, float (&r)[8], float (&i)[8]) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f2 v2 = base[rowoff + 64 * q];
            r[q] = v2.x * wr[q] - v2.y * wi[q];
            i[q] = v2.x * wi[q] + v2.y * wr[q];
        }
        fft512_wave<-1>(r, i, j, t5, lds);
    };
    for (int f = 0; f < d.nf; ++f) {
        const long off = ((long)item * d.nf + f) * d.n;
        float r[8], i[8];
        load_spec(A + off, r, i);
        if (BWD && want_gh) {
            float xr[8], xi[8];
            load_spec(Ax + off, xr, xi);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                pr[q] += xr[q] * r[q] + xi[q] * i[q];
                pi[q] += xr[q] * i[q] - xi[q] * r[q];
            }
        }
        if (!BWD || want_out) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float t = r[q] * hr[q] - i[q] * hi[q];
                i[q] = r[q] * hi[q] + i[q] * hr[q];
                r[q] = t;
            }
            fft512_wave<1>(r, i, j, t5, lds);
            f2* o = A + off;
#pragma unroll
            for (int q = 0; q < 8; ++q) o[rowoff + 64 * q] = f2{r[q] * wr[q] + i[q] * wi[q], i[q] * wr[q] - r[q] * wi[q]};
        }
    }
    if (BWD && want_gh) {
        f2* o = Pout + (long)item * d.n;
#pragma unroll
        for (int q = 0; q < 8; ++q) o[rowoff + 64 * q] = f2{pr[q], pi[q]};
    }
}

// Inverse column pass, A[frame][ja][jb] (after the row pass: ja is a time index again) -> rows 2f (real) and 2f + 1 (imaginary).
// grid (n / 8192 column tiles, frames), 1024 threads. Samples tt < limit are stored; the scale 1 / n was applied in the row pass.
__global__ __launch_bounds__(FdGeom::T) void fdfir_cols_kernel(const f2* __restrict__ W, const f2* __restrict__ tw, float* __restrict__ out, FdDims d,
                                                               int rowlen, int limit) {
    __shared__ f2 lds[FdGeom::LDS];
    const ColCfg g = col_config<FD_LOG>(d.logNA, threadIdx.x);
    const int frame = blockIdx.y, item = frame / d.nf, f = frame % d.nf;
    const bool has1 = 2 * f + 1 < d.chs;
    const long row = (long)item * d.chs + 2 * f;
    const int jb = xcd_tile(blockIdx.x, gridDim.x) * g.TC + g.c;
    const f2* in = W + (long)frame * d.n;
    float r[8], i[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const f2 v = in[(long)(g.j + g.T * q) * FD_NB + jb]; r[q] = v.x; i[q] = v.y; }
    col_fft<1>(r, i, g, tw, lds);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int tt = (g.j + g.T * q) * FD_NB + jb;
        if (tt < limit) {
            out[row * rowlen + tt] = r[q];
            if (has1) out[(row + 1) * rowlen + tt] = i[q];
        }
    }
}

// gH[item][k] = w_k / n * Herm(P)[k], k = ka + NA kb <= n / 2, from P in the permuted order [ka][kb]; bin n - k sits at
// ((n - k) % NA, (n - k) / NA). grid (NA / 16, 17, items), 256 threads = a 16 x 16 tile of (ka, kb).
__global__ __launch_bounds__(256) void fdfir_gh_kernel(const f2* __restrict__ P, f2* __restrict__ gH, FdDims d) {
    const int ka = blockIdx.x * 16 + (threadIdx.x >> 4), kb = blockIdx.y * 16 + (threadIdx.x & 15);
    const int half = d.n >> 1;
    if (kb > FD_NB / 2) return;
    const int k = ka + d.NA * kb;
    if (k > half) return;
    const f2* p = P + (long)blockIdx.z * d.n;
    const int m = (d.n - k) & (d.n - 1);
    const f2 a = p[(long)ka * FD_NB + kb], b = p[(long)(m & (d.NA - 1)) * FD_NB + (m >> d.logNA)];
    const bool edge = k == 0 || k == half;
    const float w = (edge ? 0.5f : 1.f) / (float)d.n;
    gH[(long)blockIdx.z * d.bins + k] = f2{(a.x + b.x) * w, edge ? 0.f : (a.y - b.y) * w};
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {

// DASP_ERR_UNSUPPORTED: n_fft is not a power of two in [8, 2^20]; DASP_ERR_ARG: sizes out of range
int fd_dims(long rows, long T, long n_fft, long h_rows, FdDims& d) {
    if (n_fft < (1L << FD_MIN_LOG) || n_fft > (1L << FD_MAX_LOG) || (n_fft & (n_fft - 1))) return DASP_ERR_UNSUPPORTED;
    if (rows < 0 || h_rows < 0 || T < 1 || T > 0x7fffffffL || rows > 0x7fffffffL || (rows == 0) != (h_rows == 0)) return DASP_ERR_ARG;
    if (h_rows && rows % h_rows) return DASP_ERR_ARG;
    d.n = (int)n_fft; d.bins = d.n / 2 + 1;
    d.logn = 0; while ((1 << d.logn) < d.n) ++d.logn;
    d.T = (int)T;
    d.items = (int)h_rows; d.chs = h_rows ? (int)(rows / h_rows) : 1; d.nf = (d.chs + 1) / 2;
    d.logNA = d.logn > 9 ? d.logn - 9 : 0; d.NA = 1 << d.logNA;
    if (d.logn > FD_LOG && ((long)d.items * d.nf > 65535 || d.items > 65535)) return DASP_ERR_ARG;      // grid y / z of the four-step kernels
    return DASP_OK;
}
inline bool fd_small(const FdDims& d) { return d.logn <= FD_LOG; }
inline long fd_frame_floats(const FdDims& d) { return 2L * d.items * d.nf * d.n; }       // the column transforms of every frame

}  // namespace

extern "C" {

long dasp_fdfir_work_floats(long rows, long T, long n_fft, long h_rows) {
    FdDims d;
    if (fd_dims(rows, T, n_fft, h_rows, d)) return -1;
    if (fd_small(d)) return 0;
    return 2 * fd_frame_floats(d) + 2L * d.items * d.n;          // frames of gy, frames of x, P per item (the forward call needs one set of frames)
}

int dasp_fdfir_forward(const float* x, const void* H, const void* tw, float* y, float* work, long work_floats, long rows, long T, long n_fft,
                       long h_rows, void* stream) {
    FdDims d;
    const int rc = fd_dims(rows, T, n_fft, h_rows, d);
    if (rc) return rc;
    if (!rows) return DASP_OK;
    if (!x || !H || !tw || !y) return DASP_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int Tin = d.T < d.n ? d.T : d.n;
    if (fd_small(d)) {
        const int TC = FdGeom::N >> d.logn;
        hipLaunchKernelGGL(fdfir_small_kernel<false>, dim3((unsigned)((d.items + TC - 1) / TC), (unsigned)d.nf), dim3(FdGeom::T), 0, st, x, (const f2*)H,
                           (const float*)nullptr, (const f2*)tw, y, (f2*)nullptr, d, 1, 0);
        return (int)hipGetLastError();
    }
    if (!work || work_floats < fd_frame_floats(d)) return DASP_ERR_ARG;
    const unsigned frames = (unsigned)(d.items * d.nf);
    f2* A = (f2*)work;
    hipLaunchKernelGGL(fdfir_load_kernel, dim3((unsigned)(d.n / FdLoadGeom::N), frames), dim3(FdLoadGeom::T), 0, st, x, (const f2*)tw, A, d, d.T, Tin);
    hipLaunchKernelGGL(fdfir_rows_kernel<false>, dim3((unsigned)(d.NA / 8), (unsigned)d.items), dim3(FFT_T), 0, st, A, (const f2*)nullptr, (const f2*)tw,
                       (const f2*)H, (f2*)nullptr, d, 1, 0);
    hipLaunchKernelGGL(fdfir_cols_kernel, dim3((unsigned)(d.n / FdGeom::N), frames), dim3(FdGeom::T), 0, st, (const f2*)A, (const f2*)tw, y, d, d.n, d.n);
    return (int)hipGetLastError();
}

int dasp_fdfir_backward(const float* x, const void* H, const float* gy, const void* tw, float* gx, void* gH, float* work, long work_floats,
                        long rows, long T, long n_fft, long h_rows, void* stream) {
    FdDims d;
    const int rc = fd_dims(rows, T, n_fft, h_rows, d);
    if (rc) return rc;
    if (!rows) return DASP_OK;
    if (!H || !gy || !tw || (!gx && !gH) || (gH && !x)) return DASP_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int Tin = d.T < d.n ? d.T : d.n;
    if (!fd_small(d) && (!work || work_floats < dasp_fdfir_work_floats(rows, T, n_fft, h_rows))) return DASP_ERR_ARG;
    if (gx && d.T > d.n) {                       // samples cropped by the forward transform: gradient 0
        const hipError_t e = zero_async(gx, sizeof(float) * (size_t)rows * d.T, st);
        if (e != hipSuccess) return (int)e;
    }
    if (fd_small(d)) {
        const int TC = FdGeom::N >> d.logn;
        hipLaunchKernelGGL(fdfir_small_kernel<true>, dim3((unsigned)((d.items + TC - 1) / TC), 1), dim3(FdGeom::T), 0, st, x, (const f2*)H, gy,
                           (const f2*)tw, gx, (f2*)gH, d, gx ? 1 : 0, gH ? 1 : 0);
        return (int)hipGetLastError();
    }
    const unsigned frames = (unsigned)(d.items * d.nf);
    f2* Ag = (f2*)work;
    f2* Ax = Ag + fd_frame_floats(d) / 2;
    f2* P = Ax + fd_frame_floats(d) / 2;
    const dim3 lgrid((unsigned)(d.n / FdLoadGeom::N), frames);
    hipLaunchKernelGGL(fdfir_load_kernel, lgrid, dim3(FdLoadGeom::T), 0, st, gy, (const f2*)tw, Ag, d, d.n, d.n);
    if (gH) hipLaunchKernelGGL(fdfir_load_kernel, lgrid, dim3(FdLoadGeom::T), 0, st, x, (const f2*)tw, Ax, d, d.T, Tin);
    hipLaunchKernelGGL(fdfir_rows_kernel<true>, dim3((unsigned)(d.NA / 8), (unsigned)d.items), dim3(FFT_T), 0, st, Ag, (const f2*)Ax, (const f2*)tw,
                       (const f2*)H, P, d, gx ? 1 : 0, gH ? 1 : 0);
    if (gx) hipLaunchKernelGGL(fdfir_cols_kernel, dim3((unsigned)(d.n / FdGeom::N), frames), dim3(FdGeom::T), 0, st, (const f2*)Ag, (const f2*)tw, gx, d, d.T, Tin);
    if (gH) hipLaunchKernelGGL(fdfir_gh_kernel, dim3((unsigned)(d.NA / 16), FD_NB / 32 + 1, (unsigned)d.items), dim3(256), 0, st, (const f2*)P, (f2*)gH, d);
    return (int)hipGetLastError();
}

}  // extern "C"
