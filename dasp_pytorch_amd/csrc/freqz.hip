// Frequency response of a cascade of rational sections, evaluated on the rFFT grid, and its adjoint.
// Replaces dasp_pytorch/signal.py:7-11 (fft_freqz) and :14-32 (fft_sosfreqz), which take two zero-padded rFFTs per section.
//
//   H_k = prod_s B_s(z_k) / A_s(z_k),  z_k = e^{-2 pi i k / n},  k = 0 .. n/2,
//   B_s(z) = sum_{j < Kb} b_{s,j} z^j,  A_s(z) = sum_{j < Ka} a_{s,j} z^j   (taps j >= n are cropped, as torch.fft.rfft crops its input).
//
// Layout: b (rows, S, Kb), a (rows, S, Ka) contiguous, float (f64 = 0) or double (f64 = 1); H and its cotangent gH (rows, n/2 + 1)
// interleaved complex of the same precision; gb, ga like b, a. Everything inside is fp64: for a pole close to the unit circle A(z) is
// the small difference of O(1) terms, and fp32 twiddles alone put ~1e-3 relative error into H there.
//
// Forward: one thread per bin. It takes its twiddle once (sincospi of the exactly reduced argument 2k mod 2n over n) and evaluates
// every section of FZ_ROWS rows by Horner's rule; N = prod B_s and D = prod A_s are divided once. The coefficients of a row are the
// same for every thread of the workgroup (uniform loads). Stores are one complex value per (row, bin), coalesced along the bins.
//
// Backward (two launches, no float atomics: bit-identical run to run):
//   dH/db_{s,j} =  z^j prod_{t != s} B_t / D,   dH/da_{s,j} = -z^j H / A_s,
//   grad c = sum_k Re(conj(dH_k/dc) g_k)   (torch's convention for a real input and a complex output).
// prod_{t != s} B_t is prefix x suffix: never B_s divided out (the RBJ low / high pass puts an exact zero of B on the unit circle, at
// Nyquist / DC, which is a bin at even n). 1) fz_bwd_kernel: one wave per workgroup, `tiles` x 64 consecutive bins of one row; each
// lane accumulates the S (Kb + Ka) terms of its bins in its own column of LDS (terms have a runtime count: LDS, not a register array
// with dynamic indices), then the wave sums each term's column in a fixed order and writes one fp64 partial per (row, workgroup, term).
// 2) fz_finalize_kernel: one thread per (row, coefficient) sums the partials of the row's workgroups in order.
#include <hip/hip_runtime.h>

namespace {

// C-ABI status codes (include/dasp_hip.h)
constexpr int DASP_OK = 0, DASP_ERR_ARG = -1, DASP_ERR_UNSUPPORTED = -2;

constexpr int FZ_THREADS = 256;       // forward: bins per workgroup
constexpr int FZ_ROWS = 8;            // forward: rows per workgroup at most (the twiddle is shared by them)
constexpr int FZ_MAX_S = 16;
constexpr int FZ_MAX_K = 32;
constexpr int FZ_MAX_TERMS = 96;      // S (Kb + Ka) after cropping: 16 biquads, or one section of 32 + 32 taps
constexpr int FZ_MAX_TILES = 16;      // backward: 64-bin tiles per workgroup at most
constexpr int FZ_GRID_Y = 65535;

struct cd {
    double x, y;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return {fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }
__device__ __forceinline__ cd conj(cd a) { return {a.x, -a.y}; }
__device__ __forceinline__ cd cinv(cd a) {
    const double r = 1.0 / fma(a.x, a.x, a.y * a.y);
    return {a.x * r, -a.y * r};
}

// z_k = e^{-2 pi i k / n}; 2k mod 2n is exact in integers, so the only rounding before sincospi is that of one division
__device__ __forceinline__ cd twiddle(long k, long n) {
    const double t = (double)((2 * k) % (2 * n)) / (double)n;
    double s, c;
    sincospi(t, &s, &c);
    return {c, -s};
}

// sum_{j < K} c[j] z^j by Horner's rule
template <typename T>
__device__ __forceinline__ cd horner(const T* __restrict__ c, int K, cd z) {
    cd acc = {(double)c[K - 1], 0.0};
    for (int j = K - 2; j >= 0; --j) {
        acc = cmul(acc, z);
        acc.x += (double)c[j];
    }
    return acc;
}

template <typename T>
struct cplx;
template <>
struct cplx<float> {
    using type = float2;
};
template <>
struct cplx<double> {
    using type = double2;
};

template <typename T>
__global__ void __launch_bounds__(FZ_THREADS)
fz_fwd_kernel(const T* __restrict__ b, const T* __restrict__ a, typename cplx<T>::type* __restrict__ H, int rows, int S, int Kb, int Ka,
              int Kbe, int Kae, long n, long nbins, int rpg) {
    const long k = (long)blockIdx.x * FZ_THREADS + threadIdx.x;
    if (k >= nbins) return;
    const cd z = twiddle(k, n);
    for (int g = blockIdx.y; g * rpg < rows; g += gridDim.y) {
        const int r1 = min(rows, (g + 1) * rpg);
        for (int r = g * rpg; r < r1; ++r) {
            cd N = {1.0, 0.0}, D = {1.0, 0.0};
            for (int s = 0; s < S; ++s) {
                N = cmul(N, horner(b + ((long)r * S + s) * Kb, Kbe, z));
                D = cmul(D, horner(a + ((long)r * S + s) * Ka, Kae, z));
            }
            const cd h = cmul(N, cinv(D));
            typename cplx<T>::type o;
            o.x = (T)h.x;
            o.y = (T)h.y;
            H[(long)r * nbins + k] = o;
        }
    }
}

// LDS of the backward kernel: the term accumulators, 64 doubles per term, lane l of term t at column l ^ (t & 63) (the final pass reads
// a term per lane: the swizzle keeps both access patterns free of bank conflicts), then the suffix products, 64 per section
__host__ __device__ constexpr long fz_bwd_lds_bytes(int nterm, int S) { return (long)nterm * 64 * 8 + (long)S * 64 * 16; }

template <typename T>
__global__ void __launch_bounds__(64)
fz_bwd_kernel(const T* __restrict__ b, const T* __restrict__ a, const typename cplx<T>::type* __restrict__ gH, double* __restrict__ partials,
              int S, int Kb, int Ka, int Kbe, int Kae, long n, long nbins, int tiles, int nwg) {
    extern __shared__ double fz_lds[];
    const int lane = threadIdx.x, nterm = S * (Kbe + Kae);
    double* acc = fz_lds;
    cd* q = reinterpret_cast<cd*>(fz_lds + (long)nterm * 64);
    const int row = blockIdx.x / nwg, wg = blockIdx.x % nwg;     // 1-D grid: no limit of 65535 rows
    for (int t = 0; t < nterm; ++t) acc[t * 64 + (lane ^ (t & 63))] = 0.0;
    const T* br = b + (long)row * S * Kb;
    const T* ar = a + (long)row * S * Ka;
    // the lane's twiddle for the first tile from sincospi, the next tiles' by the rotation e^{-2 pi i 64 / n} (at most 15 steps: a few
    // ulp; a sincospi per tile would keep its polynomial constants in scalar registers across the loop and spill them)
    const long k0 = (long)wg * tiles * 64 + lane;
    cd z = twiddle(k0, n);
    const cd rot = twiddle(64, n);
    for (int tile = 0; tile < tiles; ++tile, z = cmul(z, rot)) {
        const long k = k0 + (long)tile * 64;
        if (k >= nbins) break;
        const cd zc = conj(z);
        const typename cplx<T>::type gv = gH[(long)row * nbins + k];
        const cd g = {(double)gv.x, (double)gv.y};
        // suffix products of the numerators (q[s] = prod_{t > s} B_t), N and D
        cd Q = {1.0, 0.0}, D = {1.0, 0.0};
        for (int s = S - 1; s >= 0; --s) {
            q[s * 64 + lane] = Q;
            Q = cmul(Q, horner(br + s * Kb, Kbe, z));
            D = cmul(D, horner(ar + s * Ka, Kae, z));
        }
        const cd iD = cinv(D), h = cmul(Q, iD);
        const cd gD = cmul(g, conj(iD));          // conj(1 / D) g
        cd hv = cmul(conj(h), g);                 // -conj(H) g
        hv.x = -hv.x;
        hv.y = -hv.y;
        cd pre = {1.0, 0.0};
        int t0 = 0;
        for (int s = 0; s < S; ++s) {
            const cd Bs = horner(br + s * Kb, Kbe, z), As = horner(ar + s * Ka, Kae, z);
            const cd u = cmul(conj(cmul(pre, q[s * 64 + lane])), gD);    // conj(dH/db_{s,0}) g
            const cd v = cmul(conj(cinv(As)), hv);                       // conj(dH/da_{s,0}) g
            cd w = {1.0, 0.0};                                           // conj(z)^j
#pragma unroll 1
            for (int j = 0; j < Kbe; ++j, ++t0) {
                double& c = acc[t0 * 64 + (lane ^ (t0 & 63))];
                c = fma(w.x, u.x, fma(-w.y, u.y, c));
                w = cmul(w, zc);
            }
            w = {1.0, 0.0};
#pragma unroll 1
            for (int j = 0; j < Kae; ++j, ++t0) {
                double& c = acc[t0 * 64 + (lane ^ (t0 & 63))];
                c = fma(w.x, v.x, fma(-w.y, v.y, c));
                w = cmul(w, zc);
            }
            pre = cmul(pre, Bs);
        }
    }
    __syncthreads();
    double* out = partials + ((long)row * nwg + wg) * nterm;
    for (int t = lane; t < nterm; t += 64) {
        double sum = 0.0;
        for (int l = 0; l < 64; ++l) sum += acc[t * 64 + (l ^ (t & 63))];
        out[t] = sum;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
fz_finalize_kernel(const double* __restrict__ partials, T* __restrict__ gb, T* __restrict__ ga, int rows, int S, int Kb, int Ka, int Kbe,
                   int Kae, int nwg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = S * (Kb + Ka);
    if (i >= (long)rows * per) return;
    const int row = (int)(i / per), c = (int)(i % per), s = c / (Kb + Ka), j = c % (Kb + Ka);
    const bool isb = j < Kb;
    const int jj = isb ? j : j - Kb;
    double sum = 0.0;
    if (jj < (isb ? Kbe : Kae)) {                // a cropped tap (j >= n) does not reach the output: gradient 0
        const int nterm = S * (Kbe + Kae), t = s * (Kbe + Kae) + (isb ? jj : Kbe + jj);
        const double* p = partials + (long)row * nwg * nterm + t;
        for (int w = 0; w < nwg; ++w) sum += p[(long)w * nterm];
    }
    if (isb)
        gb[((long)row * S + s) * Kb + jj] = (T)sum;
    else
        ga[((long)row * S + s) * Ka + jj] = (T)sum;
}

struct FzPlan {
    int Kbe, Kae, nterm, tiles, nwg;
    long nbins;
};

// -1: arguments out of range, -2: more terms than the backward kernel's LDS holds
int fz_plan(int rows, int S, int Kb, int Ka, long n, FzPlan& p) {
    if (rows < 0 || S < 1 || S > FZ_MAX_S || Kb < 1 || Ka < 1 || Kb > FZ_MAX_K || Ka > FZ_MAX_K || n < 1) return DASP_ERR_ARG;
    p.Kbe = (int)(Kb < n ? Kb : n);
    p.Kae = (int)(Ka < n ? Ka : n);
    p.nterm = S * (p.Kbe + p.Kae);
    if (p.nterm > FZ_MAX_TERMS) return DASP_ERR_UNSUPPORTED;
    p.nbins = n / 2 + 1;
    const long tiles64 = (p.nbins + 63) / 64;
    // enough one-wave workgroups to fill the device (~16 per CU), then up to FZ_MAX_TILES tiles each: fewer partials to write and sum
    long t = ((long)rows * tiles64) / 4096;
    t = t < 1 ? 1 : t > FZ_MAX_TILES ? FZ_MAX_TILES : t;
    p.tiles = (int)t;
    p.nwg = (int)((tiles64 + t - 1) / t);
    if ((long)rows * p.nwg > 0x7fffffffL) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}

template <typename T>
int fz_forward(const T* b, const T* a, void* H, int rows, int S, int Kb, int Ka, long n, void* stream) {
    FzPlan p;
    const int rc = fz_plan(rows, S, Kb, Ka, n, p);
    if (rc) return rc;
    if (!rows) return DASP_OK;
    if (!b || !a || !H) return DASP_ERR_ARG;
    const long nbx = (p.nbins + FZ_THREADS - 1) / FZ_THREADS;
    int rpg = FZ_ROWS;                          // fewer rows per workgroup while that leaves the device short of workgroups
    while (rpg > 1 && ((rows + rpg - 1) / rpg) * nbx < 2048) rpg /= 2;
    const long groups = (rows + rpg - 1) / rpg;
    hipLaunchKernelGGL(fz_fwd_kernel<T>, dim3((unsigned)nbx, (unsigned)(groups < FZ_GRID_Y ? groups : FZ_GRID_Y)), dim3(FZ_THREADS), 0,
                       (hipStream_t)stream, b, a, reinterpret_cast<typename cplx<T>::type*>(H), rows, S, Kb, Ka, p.Kbe, p.Kae, n, p.nbins, rpg);
    return (int)hipGetLastError();
}

template <typename T>
int fz_backward(const T* b, const T* a, const void* gH, double* work, long work_doubles, T* gb, T* ga, int rows, int S, int Kb, int Ka,
                long n, void* stream) {
    FzPlan p;
    const int rc = fz_plan(rows, S, Kb, Ka, n, p);
    if (rc) return rc;
    if (!rows) return DASP_OK;
    if (!b || !a || !gH || !work || !gb || !ga || work_doubles < (long)rows * p.nwg * p.nterm) return DASP_ERR_ARG;
    hipLaunchKernelGGL(fz_bwd_kernel<T>, dim3((unsigned)((long)rows * p.nwg)), dim3(64), (unsigned)fz_bwd_lds_bytes(p.nterm, S), (hipStream_t)stream, b, a,
                       reinterpret_cast<const typename cplx<T>::type*>(gH), work, S, Kb, Ka, p.Kbe, p.Kae, n, p.nbins, p.tiles, p.nwg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const long total = (long)rows * S * (Kb + Ka);
    hipLaunchKernelGGL(fz_finalize_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, work, gb, ga, rows, S,
                       Kb, Ka, p.Kbe, p.Kae, p.nwg);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long dasp_freqz_work_doubles(int rows, int S, int Kb, int Ka, long n_fft) {
    FzPlan p;
    const int rc = fz_plan(rows, S, Kb, Ka, n_fft, p);
    return rc ? rc : (long)rows * p.nwg * p.nterm;
}

int dasp_freqz_forward(const void* b, const void* a, int rows, int S, int Kb, int Ka, long n_fft, int f64, void* H, void* stream) {
    return f64 ? fz_forward((const double*)b, (const double*)a, H, rows, S, Kb, Ka, n_fft, stream)
               : fz_forward((const float*)b, (const float*)a, H, rows, S, Kb, Ka, n_fft, stream);
}

int dasp_freqz_backward(const void* b, const void* a, const void* gH, int rows, int S, int Kb, int Ka, long n_fft, int f64, double* work,
                        long work_doubles, void* gb, void* ga, void* stream) {
    return f64 ? fz_backward((const double*)b, (const double*)a, gH, work, work_doubles, (double*)gb, (double*)ga, rows, S, Kb, Ka, n_fft, stream)
               : fz_backward((const float*)b, (const float*)a, gH, work, work_doubles, (float*)gb, (float*)ga, rows, S, Kb, Ka, n_fft, stream);
}

}  // extern "C"
