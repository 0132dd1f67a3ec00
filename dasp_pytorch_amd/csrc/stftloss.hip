// Multi-resolution STFT loss (spectral convergence + log-magnitude L1 per resolution, mean over resolutions), forward and the
// gradients with respect to either signal (the first: the chain's output at every call site of the reference; the second - auraloss
// differentiates both - through the same kernels with the signals swapped, see grad_bin): the op directly downstream of the effect chain in the reference's training loops
// (auraloss.freq.MultiResolutionSTFTLoss(), call sites examples/style_transfer.py:341,363, auto_eq.py:252, virtual_analog.py:288;
// auraloss is not vendored in the reference: the algorithm of auraloss 0.4.0 with default arguments is restated in
// oracle/dasp_oracle.py:mrstft_loss, "parity unpinned").
//
// One fused kernel per direction and resolution: a 512-thread workgroup owns 4096 / n_fft frames of
// one signal row. The frames of the two signals are gathered (reflect padding, periodic Hann window zero-padded to n_fft) as ONE
// complex signal p + i t and transformed - frames of 512 / 1024 / 2048 points (the default resolutions) as 1 / 2 / 4 interleaved
// 512-point transforms, one per wave, with at most one workgroup barrier (split kernels, below); any other power of two with col_fft
// (fft_lds.hpp: frames side by side in registers + LDS; 8192 points: one frame per 1024-thread workgroup) -, split into the two
// one-sided spectra through the mirrored bin, reduced to the four sums of a resolution
//   S1 = sum (|T| - |P|)^2,  S2 = sum |T|^2,  S3 = sum |log|P| - log|T||,  S4 = sum ||T| - |P||       (|.| = sqrt(max(re^2 + im^2, eps)))
// per workgroup; a finalize kernel adds them in fp64:  loss = mean_r( w_sc sqrt(S1)/sqrt(S2) + w_lm S3 / count + w_lin S4 / count ),
// weights (1, 1, 0) by default. The A-weighting FIR of auraloss's perceptual weighting has kernels of its own (end of the file).
// Backward recomputes the spectra, forms dL/d|P| * P/|P| on the one-sided bins, runs the inverse transform of that half spectrum and
// scatters window * Re(.) back through the frame overlap and the reflect padding with float atomics (each sample receives
// ~n_fft/hop contributions; the summation order, and only that, is not deterministic). Spectrograms never exist in HBM.
#include "common.hpp"
#include "fft_lds.hpp"

#include <cmath>

namespace dasp {

constexpr int SL_MAXRES = 8;
struct StftRes { int logF, hop, win, frames; };
// w_sc, w_lm, w_lin: the term weights of auraloss (spectral convergence, log-magnitude L1, linear-magnitude L1); a weight of exactly 0
// drops its term from the loss and from the gradient (auraloss: `... if self.w_sc else 0.0`), so w_sc = 0 with a silent target stays finite
struct StftSpec { StftRes r[SL_MAXRES]; int nres, groups; float eps, w_sc, w_lm, w_lin; };
// frames of one resolution per workgroup: 4096 / n_fft up to 4096 points, one 8192-point frame per 1024-thread workgroup
__host__ __device__ __forceinline__ int frames_per_group(int logF) { return FFT_N >> (logF < 12 ? logF : 12); }

__global__ void stft_twiddle_kernel(f2* __restrict__ tw) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < FFT_N) {
        double sn, cs;
        sincospi(2.0 * (double)e / (double)FFT_N, &sn, &cs);
        tw[e] = f2{(float)cs, (float)-sn};
    }
}

__device__ __forceinline__ int reflect_index(int s, int N) { return s < 0 ? -s : (s >= N ? 2 * N - 2 - s : s); }
// periodic Hann window of `win` samples centred in a frame of F samples (torch.stft zero-pads the window on both sides)
__device__ __forceinline__ float hann_in_frame(int n, int F, int win) {
    const int m = n - (F - win) / 2;
    return (m >= 0 && m < win) ? 0.5f - 0.5f * cospif(2.f * (float)m / (float)win) : 0.f;
}

// the two one-sided spectra of bin k from Z = FFT(p + i t): P = (Z[k] + conj Z[F-k]) / 2, T = (Z[k] - conj Z[F-k]) / (2i)
struct Bin { float pr, pi, tr, ti; };
__device__ __forceinline__ Bin split_bin(float zr, float zi, float mr, float mi) {
    return Bin{0.5f * (zr + mr), 0.5f * (zi - mi), 0.5f * (zi + mi), -0.5f * (zr - mr)};
}

// one bin's contribution to the four sums of a resolution
// torch.clamp(min = eps): a NaN power stays NaN (fmaxf would hand back eps and count the bins of a frame that holds a NaN or inf sample as silent)
__device__ __forceinline__ float clamp_min_eps(float x, float eps) { return x < eps ? eps : x; }
__device__ __forceinline__ void loss_terms(const Bin& b, float eps, float& s1, float& s2, float& s3, float& s4) {
    const float p2 = clamp_min_eps(b.pr * b.pr + b.pi * b.pi, eps), t2 = clamp_min_eps(b.tr * b.tr + b.ti * b.ti, eps);
    const float pm = __builtin_amdgcn_sqrtf(p2), tm = __builtin_amdgcn_sqrtf(t2);      // operands in [eps, ~1e6]: the plain instructions are exact enough (1 ulp)
    s1 = fmaf(tm - pm, tm - pm, s1);
    s2 += t2;
    s3 += 0.5f * fabsf(__logf(__fdividef(p2, t2)));       // |log pm - log tm| = |log(p2 / t2)| / 2; the ratio stays within 1e-14 .. 1e14
    s4 += fabsf(tm - pm);
}
// one bin of the gradient spectrum: dL/d|P| * P / |P|
// k_self: the gradient w.r.t. the SECOND signal of the loss (the kernels are then called with the two signals swapped): the spectral
// convergence term is normalised by that signal's own norm, d/d|T| (s1 / s2) = (|T| - |P|) / (s1 s2) - s1 |T| / s2^3 - the first part is what
// the swapped call computes anyway, the second is k_self = - s1 / s2^3 times the spectrum itself; the two magnitude terms are symmetric.
// Linear-magnitude L1: d/d|P| |(|T| - |P|)| = -sign(|T| - |P|), times k_lin = w_lin gl / count. Each constant carries its term's weight.
struct GradK { float sc, lm, lin, self; };
__device__ __forceinline__ GradK grad_consts(const StftSpec& spec, const float* __restrict__ stats, const float* __restrict__ gloss, int res, int wrt_second) {
    const float s1 = stats[res * 4], s2 = stats[res * 4 + 1], count = stats[res * 4 + 2];
    const float gl = gloss[0] / (float)spec.nres;
    GradK k;
    k.sc = spec.w_sc != 0.f && s1 != 0.f ? spec.w_sc * gl / (s1 * s2) : 0.f;
    k.lm = spec.w_lm * gl / count;
    k.lin = spec.w_lin * gl / count;
    k.self = wrt_second && spec.w_sc != 0.f ? -(spec.w_sc * gl) * s1 / (s2 * s2 * s2) : 0.f;
    return k;
}
// LIN: the linear-magnitude term is compiled in only where w_lin != 0 (the launch selects the instance): without it the default loss's
// backward kernels keep their register count (mrstft_bwd_split_kernel<1>: 80 VGPRs, 6 waves per SIMD; with it 82, 5 waves, 1.6 % slower)
template <bool LIN>
__device__ __forceinline__ void grad_bin(const Bin& b, float eps, const GradK& k, float& hr, float& hi) {
    hr = 0.f; hi = 0.f;
    const float praw = b.pr * b.pr + b.pi * b.pi;
    if (!(praw <= eps)) {                                        // the clamp has zero slope below eps; a NaN bin goes through, as in autograd
        const float tm = sqrtf(clamp_min_eps(b.tr * b.tr + b.ti * b.ti, eps)), pm = sqrtf(praw);
        const float sgn = tm > pm ? 1.f : (tm < pm ? -1.f : 0.f);            // sign(log tm - log pm)
        float d = k.sc * (pm - tm) - k.lm * sgn / pm;
        if constexpr (LIN) d -= k.lin * sgn;
        const float gm = d / pm + k.self;                                    // dL/d|P| / |P|
        hr = gm * b.pr; hi = gm * b.pi;
    }
}

// gather + window + forward transform of this thread's 8 samples of its frame; afterwards r/i = Z[j + T q] and mr/mi = Z[F - (j + T q)]
// the window of a resolution, once per workgroup (all its frames share it): wlds[n] = hann_in_frame(n), n < F; a barrier follows in the caller's path
template <int NT = 512>
__device__ __forceinline__ void window_to_lds(float* wlds, const StftRes& R) {
    const int F = 1 << R.logF;
    for (int n = threadIdx.x; n < F; n += NT) wlds[n] = hann_in_frame(n, F, R.win);
    __syncthreads();
}

template <int LOGN>
__device__ __forceinline__ void frames_to_spectra(const float* __restrict__ prow, const float* __restrict__ trow, int N, int frame, bool live,
                                                  const StftRes& R, const ColCfg& g, const f2* __restrict__ tw, f2* lds, const float* wlds,
                                                  float (&r)[8], float (&i)[8], float (&mr)[8], float (&mi)[8]) {
    const int F = 1 << R.logF;
    // all 16 loads first, at indices that are always valid (a load under `if (w != 0)` is a branch with its own wait: 8 exposed round
    // trips per thread); the window, zero outside its support and for frames past the end, is applied afterwards
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int s = reflect_index(frame * R.hop - F / 2 + g.j + g.T * q, N);
        s = s < 0 ? 0 : (s >= N ? N - 1 : s);
        r[q] = prow[s]; i[q] = trow[s];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float w = live ? wlds[g.j + g.T * q] : 0.f;
        r[q] *= w; i[q] *= w;
    }
    col_fft<-1, LOGN>(r, i, g, tw, lds);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[fft_pad(g.j + g.T * q) * g.TC + g.c] = f2{r[q], i[q]};
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f2 m = lds[fft_pad((F - (g.j + g.T * q)) & (F - 1)) * g.TC + g.c];
        mr[q] = m.x; mi[q] = m.y;
    }
    __syncthreads();       // the caller may reuse lds for another transform
}

// One launch per resolution. These two kernels take any power of two 8 .. 4096 (LOGN = 12: col_fft with run-time geometry in a
// 512-thread workgroup) and 8192 (LOGN = 13: one frame per 1024-thread workgroup, 8 points per thread, four radix-8 passes and a radix-2
// pass); frames of 512, 1024 and 2048 points - the default resolutions - run the split kernels further down.
// partials[((res * rows + row) * groups + group) * 4 + {0, 1, 2, 3}]
template <int LOGN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, float* __restrict__ partials,
                  StftSpec spec, int N, int res) {
    constexpr int NT = ColGeom<LOGN>::T, NW = NT / 64;
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    __shared__ float red[NW][4];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;                  // the only size this instance runs: compile-time geometry
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int row = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;          // uniform: this resolution has fewer frame groups than the grid
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<NT>(wlds, R);
    float r[8], i[8], mr[8], mi[8];
    frames_to_spectra<LOGN>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, R, g, tw, lds, wlds, r, i, mr, mi);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q;
        if (live && k <= F / 2) {
            loss_terms(split_bin(r[q], i[q], mr[q], mi[q]), spec.eps, s1, s2, s3, s4);
        }
    }
    s1 = wave_sum_uniform(s1); s2 = wave_sum_uniform(s2); s3 = wave_sum_uniform(s3); s4 = wave_sum_uniform(s4);
    if (lane_id() == 0) { red[wave_id()][0] = s1; red[wave_id()][1] = s2; red[wave_id()][2] = s3; red[wave_id()][3] = s4; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float a = 0.f;
        for (int v = 0; v < NW; ++v) a += red[v][threadIdx.x];
        partials[(((size_t)res * gridDim.y + row) * spec.groups + blockIdx.x) * 4 + threadIdx.x] = a;
    }
}
// step 1, one workgroup per (half, resolution, sum): stats[(half * nres + res) * 4 + c] = S_c, added up in fp64; the mono loss has one
// half, the sum / difference loss two (gridDim.x = halves * nres * 4). 16 waves walk the rows (items), the lanes the frame groups of a row,
// four loads in flight per lane (one thread per element with an index division: 17 us; this: ~5)
__global__ void __launch_bounds__(1024)
mrstft_reduce_kernel(const float* __restrict__ partials, StftSpec spec, int rows, float* __restrict__ stats) {
    __shared__ double red[16];
    const int hr = blockIdx.x / 4, c = blockIdx.x % 4, res = hr % spec.nres, l = lane_id(), wv = wave_id();
    const int TC = frames_per_group(spec.r[res].logF), ng = (spec.r[res].frames + TC - 1) / TC;
    double s = 0.0;
    for (int row = wv; row < rows; row += 16) {
        const float* p = partials + ((size_t)hr * rows + row) * spec.groups * 4 + c;
        for (int g0 = l; g0 < ng; g0 += 256) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int gi = g0 + 64 * u; v[u] = p[(size_t)(gi < ng ? gi : ng - 1) * 4]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) s += g0 + 64 * u < ng ? (double)v[u] : 0.0;
        }
    }
    s = wave_sum(s);
    if (l == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int v = 0; v < 16; ++v) t += red[v];
        stats[hr * 4 + c] = (float)t;
    }
}
// step 2, thread h < halves for half h: stats[(h * nres + res) * 4 ..] = (sqrt S1, sqrt S2, count, S3); loss[h] = mean over resolutions of
// w_sc sqrt(S1)/sqrt(S2) + w_lm S3/count + w_lin S4/count, a term with weight 0 left out. count = rows x frames x (n_fft / 2 + 1), or
// rows x frames x n_bins on mel-scaled magnitudes (nbins > 0)
__global__ void mrstft_finalize_kernel(StftSpec spec, int rows, int nbins, int halves, float* __restrict__ stats, float* __restrict__ loss) {
    if ((int)threadIdx.x >= halves) return;
    const int half = threadIdx.x;
    float* st = stats + half * spec.nres * 4;
    double total = 0.0;
    for (int res = 0; res < spec.nres; ++res) {
        const double F = (double)(1 << spec.r[res].logF);
        const double count = (double)rows * spec.r[res].frames * (nbins > 0 ? (double)nbins : F / 2 + 1);
        const double s1 = sqrt((double)st[res * 4 + 0]), s2 = sqrt((double)st[res * 4 + 1]), s3 = (double)st[res * 4 + 2];
        const double s4 = (double)st[res * 4 + 3];
        st[res * 4 + 0] = (float)s1; st[res * 4 + 1] = (float)s2; st[res * 4 + 2] = (float)count; st[res * 4 + 3] = (float)s3;
        double l = 0.0;
        if (spec.w_sc != 0.f) l += (double)spec.w_sc * (s1 / s2);
        if (spec.w_lm != 0.f) l += (double)spec.w_lm * (s3 / count);
        if (spec.w_lin != 0.f) l += (double)spec.w_lin * (s4 / count);
        total += l;
    }
    loss[half] = (float)(total / spec.nres);
}

// gpred (rows, N) must be zero on entry; gloss = d(objective)/d(loss), a device scalar
template <int LOGN, bool LIN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, const float* __restrict__ stats,
                  const float* __restrict__ gloss, float* __restrict__ gpred, StftSpec spec, int N, int res, int wrt_second) {
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int row = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<ColGeom<LOGN>::T>(wlds, R);
    float r[8], i[8], mr[8], mi[8];
    frames_to_spectra<LOGN>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, R, g, tw, lds, wlds, r, i, mr, mi);
    const GradK kk = grad_consts(spec, stats, gloss, res, wrt_second);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q;
        float hr = 0.f, hi = 0.f;
        if (live && k <= F / 2) grad_bin<LIN>(split_bin(r[q], i[q], mr[q], mi[q]), spec.eps, kk, hr, hi);
        r[q] = hr; i[q] = hi;
    }
    col_fft<1, LOGN>(r, i, g, tw, lds);                                    // sum_k H[k] e^{+2 pi i k n / F}, H = 0 on the upper half
    float* grow = gpred + (size_t)row * N;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = g.j + g.T * q;
        const float w = hann_in_frame(n, F, R.win);     // measured: reading the LDS table here instead costs 7 % of the kernel
        if (live && w != 0.f) atomicAdd(grow + reflect_index(frame * R.hop - F / 2 + n, N), w * r[q]);
    }
}

// ---- n_fft = 512 R, R = 1, 2, 4: R waves per frame ------------------------------------------------------------------------------------
// A frame of F = 512 R points is R interleaved 512-point transforms (decimation in frequency): y_r'[m] = W_F^(m r') sum_rho x[m + 512 rho]
// W_R^(rho r'), X[r' + R kappa] = FFT512(y_r')[kappa]. Thread u of a frame (64 R threads, lanes along consecutive samples: coalesced gather
// and scatter) holds x[m + 512 rho] for 8 / R values of m, does the radix-R step in registers, and one transpose through LDS (the only
// workgroup barrier of the transform; none for R = 1) hands wave r' its y_r', which it transforms on its own (fft512_wave: wave-private
// exchanges). Afterwards lane l, register s of wave r' holds bin k = r' + R (l + 64 s). The one-sided bins k <= F / 2 are exactly the
// registers s < 4 of every wave (plus bin F / 2 in lane 0 of wave 0), so no lane idles through the logarithms, and the mirrored bin F - k
// sits in registers 7 - s of wave (R - r') % R, lane 63 - l (wave 0: lane 64 - l; its lane 0 keeps bin 0): lane permutes when that is the
// same wave (R = 1, 2), one more exchange of the upper registers through LDS for R = 4. 8 / R frames per workgroup, as the generic
// kernels group them (they remain for every other power of two).
template <int R> struct SplitCfg {
    int l, wv, c, rp, u;
    __device__ __forceinline__ SplitCfg() { l = lane_id(); wv = wave_id(); c = wv / R; rp = wv % R; u = rp * 64 + l; }
};

// forward: r/i <- this wave's bins, mr/mi <- the mirrored bins of registers 0..3
template <int R>
__device__ __forceinline__ void split_frame_spectrum(const float* __restrict__ prow, const float* __restrict__ trow, int N, int frame, bool live,
                                                     const StftRes& Rs, const SplitCfg<R>& g, const f2* __restrict__ tw, const Fft512Tw& t5,
                                                     f2* lds, const float* wlds, float (&r)[8], float (&i)[8], float (&mr)[4], float (&mi)[4]) {
    constexpr int F = 512 * R, G = 8 / R;
    f2* row = lds + g.wv * FFT512_LDS;
#pragma unroll
    for (int q = 0; q < 8; ++q) {              // register q = gi * R + rho  <->  sample n = (u + 64 R gi) + 512 rho
        const int n = g.u + 64 * R * (q / R) + 512 * (q % R);
        int s = reflect_index(frame * Rs.hop - F / 2 + n, N);
        s = s < 0 ? 0 : (s >= N ? N - 1 : s);
        r[q] = prow[s]; i[q] = trow[s];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float w = live ? wlds[g.u + 64 * R * (q / R) + 512 * (q % R)] : 0.f;
        r[q] *= w; i[q] *= w;
    }
    if constexpr (R > 1) {
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            const int m = g.u + 64 * R * gi;
            if constexpr (R == 2) {
                const float ar = r[2 * gi], ai = i[2 * gi];
                r[2 * gi] = ar + r[2 * gi + 1]; i[2 * gi] = ai + i[2 * gi + 1];
                r[2 * gi + 1] = ar - r[2 * gi + 1]; i[2 * gi + 1] = ai - i[2 * gi + 1];
            } else {
                dft4<-1>(r[4 * gi], i[4 * gi], r[4 * gi + 1], i[4 * gi + 1], r[4 * gi + 2], i[4 * gi + 2], r[4 * gi + 3], i[4 * gi + 3]);
            }
#pragma unroll
            for (int k = 1; k < R; ++k) {
                const f2 w = tw[m * k * (8 / R)];                       // W_F^(m k): m k < F, table step 4096 / F
                cmul_dir<-1>(r[R * gi + k], i[R * gi + k], w.x, w.y);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) lds[(g.c * R + k) * FFT512_LDS + m] = f2{r[R * gi + k], i[R * gi + k]};
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) { const f2 v = row[g.l + 64 * q]; r[q] = v.x; i[q] = v.y; }
    }
    fft512_wave<-1>(r, i, g.l, t5, row);
    if constexpr (R == 4) {
        // the upper registers of every wave through LDS: wave r' reads those of wave (4 - r') % 4
        wave_lds_sync();
#pragma unroll
        for (int s = 4; s < 8; ++s) row[g.l + 64 * s] = f2{r[s], i[s]};
        __syncthreads();
        const f2* prow2 = lds + (g.c * R + ((R - g.rp) & (R - 1))) * FFT512_LDS;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kap = g.l + 64 * s;
            const f2 v = prow2[g.rp == 0 ? ((512 - kap) & 511) : 511 - kap];
            const bool self = g.rp == 0 && kap == 0;                    // bin 0 mirrors onto itself (and was not published)
            mr[s] = self ? r[0] : v.x; mi[s] = self ? i[0] : v.y;
        }
        __syncthreads();                                                // the rows are reused (inverse transform / next exchange)
    } else {
        // same wave: wave 0 (and R = 1) pairs lane l with lane 64 - l, its lane 0 with its own registers; wave 1 of R = 2 pairs l with 63 - l
        const bool w0 = g.rp == 0;
        const int src = w0 ? ((64 - g.l) & 63) : 63 - g.l;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float zr = __shfl(r[7 - s], src), zi = __shfl(i[7 - s], src);
            const bool own = w0 && g.l == 0;
            mr[s] = own ? r[(8 - s) & 7] : zr;
            mi[s] = own ? i[(8 - s) & 7] : zi;
        }
    }
}

template <int R>
__global__ void __launch_bounds__(512)
mrstft_fwd_split_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, float* __restrict__ partials,
                        StftSpec spec, int N, int res) {
    __shared__ f2 lds[8 * FFT512_LDS];
    __shared__ float wlds[512 * R];
    __shared__ float red[8][4];
    const StftRes Rs = spec.r[res];
    const SplitCfg<R> g;
    const int row = blockIdx.y;
    const int frame = blockIdx.x * (8 / R) + g.c;
    const bool live = frame < Rs.frames;
    window_to_lds(wlds, Rs);
    const Fft512Tw t5 = fft512_twiddles(g.l, tw);
    float r[8], i[8], mr[4], mi[4];
    split_frame_spectrum<R>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, Rs, g, tw, t5, lds, wlds, r, i, mr, mi);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    if (live) {
#pragma unroll
        for (int s = 0; s < 4; ++s) loss_terms(split_bin(r[s], i[s], mr[s], mi[s]), spec.eps, s1, s2, s3, s4);
        if (g.rp == 0 && g.l == 0) loss_terms(split_bin(r[4], i[4], r[4], i[4]), spec.eps, s1, s2, s3, s4);       // bin F / 2 mirrors onto itself
    }
    s1 = wave_sum_uniform(s1); s2 = wave_sum_uniform(s2); s3 = wave_sum_uniform(s3); s4 = wave_sum_uniform(s4);
    if (g.l == 0) { red[g.wv][0] = s1; red[g.wv][1] = s2; red[g.wv][2] = s3; red[g.wv][3] = s4; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float a = 0.f;
        for (int v = 0; v < 8; ++v) a += red[v][threadIdx.x];
        partials[(((size_t)res * gridDim.y + row) * spec.groups + blockIdx.x) * 4 + threadIdx.x] = a;
    }
}

template <int R, bool LIN>
__global__ void __launch_bounds__(512)
mrstft_bwd_split_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, const float* __restrict__ stats,
                        const float* __restrict__ gloss, float* __restrict__ gpred, StftSpec spec, int N, int res, int wrt_second) {
    constexpr int F = 512 * R, G = 8 / R;
    __shared__ f2 lds[8 * FFT512_LDS];
    __shared__ float wlds[512 * R];
    const StftRes Rs = spec.r[res];
    const SplitCfg<R> g;
    const int row = blockIdx.y;
    const int frame = blockIdx.x * (8 / R) + g.c;
    const bool live = frame < Rs.frames;
    window_to_lds(wlds, Rs);
    const Fft512Tw t5 = fft512_twiddles(g.l, tw);
    float r[8], i[8], mr[4], mi[4];
    f2* rowbuf = lds + g.wv * FFT512_LDS;
    split_frame_spectrum<R>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, Rs, g, tw, t5, lds, wlds, r, i, mr, mi);
    const GradK kk = grad_consts(spec, stats, gloss, res, wrt_second);
    float h4r = 0.f, h4i = 0.f;
    if (live && g.rp == 0 && g.l == 0) grad_bin<LIN>(split_bin(r[4], i[4], r[4], i[4]), spec.eps, kk, h4r, h4i);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float hr = 0.f, hi = 0.f;
        if (live) grad_bin<LIN>(split_bin(r[s], i[s], mr[s], mi[s]), spec.eps, kk, hr, hi);
        r[s] = hr; i[s] = hi;
    }
    r[4] = h4r; i[4] = h4i;
#pragma unroll
    for (int s = 5; s < 8; ++s) { r[s] = 0.f; i[s] = 0.f; }
    // x[n] = sum_k H[k] e^(+2 pi i k n / F), H = 0 above bin F / 2: the forward steps mirrored
    fft512_wave<1>(r, i, g.l, t5, rowbuf);
    if constexpr (R > 1) {
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 8; ++q) rowbuf[g.l + 64 * q] = f2{r[q], i[q]};
        __syncthreads();
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
            const int m = g.u + 64 * R * gi;
#pragma unroll
            for (int k = 0; k < R; ++k) { const f2 v = lds[(g.c * R + k) * FFT512_LDS + m]; r[R * gi + k] = v.x; i[R * gi + k] = v.y; }
#pragma unroll
            for (int k = 1; k < R; ++k) {
                const f2 w = tw[m * k * (8 / R)];
                cmul_dir<1>(r[R * gi + k], i[R * gi + k], w.x, w.y);
            }
            if constexpr (R == 2) {
                const float ar = r[2 * gi], ai = i[2 * gi];
                r[2 * gi] = ar + r[2 * gi + 1]; i[2 * gi] = ai + i[2 * gi + 1];
                r[2 * gi + 1] = ar - r[2 * gi + 1]; i[2 * gi + 1] = ai - i[2 * gi + 1];
            } else {
                dft4<1>(r[4 * gi], i[4 * gi], r[4 * gi + 1], i[4 * gi + 1], r[4 * gi + 2], i[4 * gi + 2], r[4 * gi + 3], i[4 * gi + 3]);
            }
        }
    }
    // (adding the workgroup's overlapping frames up in LDS first - float atomics on LDS, then one global atomic per sample of the span,
    // 2.5x fewer of them - was measured at +90 us per kernel: the global float atomics below are the cheaper ones)
    float* grow = gpred + (size_t)row * N;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = g.u + 64 * R * (q / R) + 512 * (q % R);
        const float w = hann_in_frame(n, F, Rs.win);
        if (live && w != 0.f) atomicAdd(grow + reflect_index(frame * Rs.hop - F / 2 + n, N), w * r[q]);
    }
}

// ---- perceptual weighting: the A-weighting FIR of auraloss (FIRFilter(filter_type="aw", ntaps=101)) -------------------------------------
// y[n] = sum_{k=0}^{K-1} h[k] x[n + k - K/2], zeros outside [0, N) (conv1d(x, h, padding=K/2)); K odd, <= 101. The taps sit centred in
// 101 LDS slots (zeros around a shorter filter, which walks its own slots only), so every output is the same ntaps fmas in the same order:
// the result does not depend on the tile it falls in, and is bit-identical run to run. flip = 1 reverses the taps: the adjoint, gx[m] = sum_k h[k] gy[m - k + K/2],
// is the same sum over h[K-1-k] (no symmetry of the taps is assumed). A workgroup of 256 threads owns FIR_TILE consecutive outputs of one
// row of one of the two signals (blockIdx.z): the tile plus a 50-sample halo on each side goes to LDS, each thread computes 8 consecutive
// outputs from its 108-sample window, the taps are LDS broadcasts.
constexpr int FIR_MAXTAPS = 101, FIR_HALO = FIR_MAXTAPS / 2, FIR_NT = 256, FIR_Q = 8, FIR_TILE = FIR_NT * FIR_Q;
__global__ void __launch_bounds__(FIR_NT)
fir_same_kernel(const float* __restrict__ x0, const float* __restrict__ x1, float* __restrict__ y0, float* __restrict__ y1,
                const float* __restrict__ taps, int ntaps, int flip, int N) {
    __shared__ float xs[FIR_TILE + 2 * FIR_HALO + 4];
    __shared__ float hs[FIR_MAXTAPS + 3];
    const int t = threadIdx.x;
    const float* x = (blockIdx.z ? x1 : x0) + (size_t)blockIdx.y * N;
    float* y = (blockIdx.z ? y1 : y0) + (size_t)blockIdx.y * N;
    const long n0 = (long)blockIdx.x * FIR_TILE;
    if (t < FIR_MAXTAPS + 3) {
        const int k = t - (FIR_HALO - ntaps / 2);
        hs[t] = (t < FIR_MAXTAPS && k >= 0 && k < ntaps) ? taps[flip ? ntaps - 1 - k : k] : 0.f;
    }
    for (int e = t; e < FIR_TILE + 2 * FIR_HALO; e += FIR_NT) {
        const long s = n0 - FIR_HALO + e;
        xs[e] = (s >= 0 && s < N) ? x[s] : 0.f;
    }
    __syncthreads();
    const float* xw = xs + FIR_Q * t;
    float acc[FIR_Q];
#pragma unroll
    for (int q = 0; q < FIR_Q; ++q) acc[q] = 0.f;
    if (ntaps == FIR_MAXTAPS) {
#pragma unroll
        for (int k = 0; k < FIR_MAXTAPS; ++k) {
            const float h = hs[k];
#pragma unroll
            for (int q = 0; q < FIR_Q; ++q) acc[q] = fmaf(h, xw[q + k], acc[q]);
        }
    } else {
        // a shorter filter walks its own slots only, in the same order: the zero slots around it add exactly 0 to a finite sum, but 0 * NaN
        // (or 0 * inf) would carry a bad sample 50 samples to either side, where conv1d confines it to ntaps outputs
        const int lo = FIR_HALO - ntaps / 2;
        for (int k = lo; k < lo + ntaps; ++k) {
            const float h = hs[k];
#pragma unroll
            for (int q = 0; q < FIR_Q; ++q) acc[q] = fmaf(h, xw[q + k], acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < FIR_Q; ++q) {
        const long n = n0 + FIR_Q * t + q;
        if (n < N) y[n] = acc[q];
    }
}
// the taps by value (kernel arguments), so that writing them to device memory is one kernel node of a captured graph, not a copy from host memory
struct FirTaps { float h[FIR_MAXTAPS]; int n; };
__global__ void fir_taps_kernel(float* __restrict__ dst, FirTaps taps) {
    if ((int)threadIdx.x < taps.n) dst[threadIdx.x] = taps.h[threadIdx.x];
}

// ---- mel-scaled magnitudes: auraloss's scale="mel" (M = W |X| per frame, W = librosa.filters.mel(sr, n_fft, n_mels), Slaney) -----------
// The sums of a resolution then run over rows x frames x n_bins of M_P = W |P|, M_T = W |T| (no clamp after the projection), and the
// gradient goes back through W^T: dL/d|P|[k] = sum_m W[m, k] dL/dM_P[m]. The filters are triangles between consecutive edge
// frequencies e[0 .. B+1], so a filter's support is a run of bins and a bin lies in at most two filters, m0 and m0 + 1. One table per
// resolution (K = n_fft / 2 + 1 bins, B filters) serves both directions:
//   f2  w[K]        the bin's weights in filters m0 and m0 + 1 (0 where that filter does not exist or does not reach the bin)
//   int m0[K]       0 .. B - 1
//   int span[B][2]  first bin and bin count of the filter's support (count 0: a filter narrower than the bin spacing)
// built on the device in fp64 from the edges, which arrive as kernel arguments (fir_taps_kernel's route: a kernel node of a captured graph).
// The kernels are mrstft_fwd_kernel / mrstft_bwd_kernel (col_fft, every power of two 8 .. 8192) with the magnitudes of the one-sided
// bins laid out in the exchange buffer, free after frames_to_spectra's last barrier, as mag[signal][bin][frame column]; the (filter, column)
// sums are then gathered over each filter's support in a fixed order (no LDS atomics: the loss is bit-identical run to run).
constexpr int MEL_MAXBINS = 256;
struct MelEdges { double e[MEL_MAXBINS + 2]; };
struct MelTab { const f2* w; const int* m0; const int* span; int B; };
__host__ __device__ __forceinline__ long mel_table_len(int F, int B) { return 3L * (F / 2 + 1) + 2L * B; }
__device__ __forceinline__ MelTab mel_tab(const float* t, int F, int B) {
    const int K = F / 2 + 1;
    return MelTab{reinterpret_cast<const f2*>(t), reinterpret_cast<const int*>(t + 2 * K), reinterpret_cast<const int*>(t + 3 * K), B};
}

__global__ void __launch_bounds__(256)
mel_table_kernel(float* __restrict__ tab, MelEdges E, double sr, int F, int B) {
    __shared__ double es[MEL_MAXBINS + 2];
    for (int n = threadIdx.x; n < B + 2; n += 256) es[n] = E.e[n];
    __syncthreads();
    const int K = F / 2 + 1;
    f2* w = reinterpret_cast<f2*>(tab);
    int* m0 = reinterpret_cast<int*>(tab + 2 * K);
    int* span = reinterpret_cast<int*>(tab + 3 * K);
    auto freq = [&](int k) { return (double)k * sr / (double)F; };
    // losses.mel_filterbank's expression, operation for operation (IEEE fp64 on both sides, nothing here can contract into an fma)
    auto weight = [&](int m, double f) {
        const double lo = (f - es[m]) / (es[m + 1] - es[m]), hi = (es[m + 2] - f) / (es[m + 2] - es[m + 1]);
        return fmax(0.0, fmin(lo, hi)) * (2.0 / (es[m + 2] - es[m]));
    };
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        const double f = freq(k);
        int lo = 0, hi = B + 1;                                  // the last edge <= f (e[0] = 0 <= f)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (es[mid] <= f) lo = mid; else hi = mid - 1;
        }
        int m = lo - 1;                                          // f in [e[lo], e[lo + 1]): the falling side of filter lo - 1, the rising side of filter lo
        m = m < 0 ? 0 : (m > B - 1 ? B - 1 : m);
        const double wa = weight(m, f), wb = m + 1 < B ? weight(m + 1, f) : 0.0;
        w[k] = f2{(float)wa, (float)wb};
        m0[k] = m;
    }
    if (blockIdx.x == 0) {
        for (int m = threadIdx.x; m < B; m += 256) {             // bins with e[m] < f_k < e[m + 2]
            const double a = es[m], b = es[m + 2];
            int k0 = (int)(a * (double)F / sr);
            k0 = k0 < 0 ? 0 : (k0 > K ? K : k0);
            while (k0 > 0 && freq(k0 - 1) > a) --k0;
            while (k0 < K && freq(k0) <= a) ++k0;
            int k1 = (int)(b * (double)F / sr);
            k1 = k1 < 0 ? 0 : (k1 > K - 1 ? K - 1 : k1);
            while (k1 < K - 1 && freq(k1 + 1) < b) ++k1;
            while (k1 >= 0 && freq(k1) >= b) --k1;
            span[2 * m] = k0 < K ? k0 : 0;
            span[2 * m + 1] = k1 >= k0 ? k1 - k0 + 1 : 0;
        }
    }
}
// the dense (B, K) matrix a table stands for, as the forward reads it: bin k of filter m inside the filter's span, 0 outside
__global__ void mel_dense_kernel(const float* __restrict__ tab, float* __restrict__ dense, int F, int B) {
    const int K = F / 2 + 1, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (k >= K) return;
    const MelTab t = mel_tab(tab, F, B);
    const int first = t.span[2 * m], cnt = t.span[2 * m + 1], mk = t.m0[k];
    const f2 w = t.w[k];
    dense[(size_t)m * K + k] = (k >= first && k < first + cnt) ? (mk == m ? w.x : (mk + 1 == m ? w.y : 0.f)) : 0.f;
}

// mag[(s K + k) TC + c] = |X_s|[k] of frame column c, s = 0 (first signal), 1 (second); consecutive threads of a q write consecutive words
template <int LOGN>
__device__ __forceinline__ void mel_magnitudes_to_lds(float* mag, const ColCfg& g, int F, float eps, const float (&r)[8], const float (&i)[8],
                                                      const float (&mr)[8], const float (&mi)[8]) {
    const int K = F / 2 + 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q;
        if (k <= F / 2) {
            const Bin b = split_bin(r[q], i[q], mr[q], mi[q]);
            mag[k * g.TC + g.c] = sqrtf(clamp_min_eps(b.pr * b.pr + b.pi * b.pi, eps));
            mag[(K + k) * g.TC + g.c] = sqrtf(clamp_min_eps(b.tr * b.tr + b.ti * b.ti, eps));
        }
    }
    __syncthreads();
}
// The B x TC sums M_s[m][c] = sum_k W[m, k] mag_s[k][c]. Items (m, c), c fastest, so the threads of a wave read one contiguous segment
// of a bin's row; where there are fewer items than threads (one 8192-point frame per workgroup, 128 filters of up to 254 bins) L = 2 .. 64
// lanes share an item, stride through the filter's support and add up by butterflies - the same order every run. fn(owner, m, c, M_P, M_T)
// is called by every thread (the shuffles in front of it need whole waves), owner true in one lane per item.
template <int NT, class Fn>
__device__ __forceinline__ void mel_filter_sums(const float* mag, int K, int TC, int logTC, const MelTab& t, Fn&& fn) {
    const int items = t.B * TC;
    int logL = 0;
    while (logL < 6 && (items << (logL + 1)) <= NT) ++logL;
    const int L = 1 << logL, sub = threadIdx.x & (L - 1), slot = threadIdx.x >> logL, nslots = NT >> logL;
    for (int base = 0; base < items; base += nslots) {                // workgroup-uniform trip count
        const int item = base + slot, m = item >> logTC, c = item & (TC - 1);
        float mp = 0.f, mt = 0.f;
        if (item < items) {
            const int first = t.span[2 * m], cnt = t.span[2 * m + 1];
            for (int s = sub; s < cnt; s += L) {
                const int k = first + s;
                const f2 w = t.w[k];
                const float wk = t.m0[k] == m ? w.x : w.y;
                mp = fmaf(wk, mag[k * TC + c], mp);
                mt = fmaf(wk, mag[(K + k) * TC + c], mt);
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) { mp += __shfl_xor(mp, o); mt += __shfl_xor(mt, o); }
        fn(item < items && sub == 0, m, c, mp, mt);
    }
}

template <int LOGN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_mel_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, const float* __restrict__ tab,
                      float* __restrict__ partials, StftSpec spec, int N, int res, int nbins) {
    constexpr int NT = ColGeom<LOGN>::T, NW = NT / 64;
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    __shared__ float red[NW][4];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int row = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<NT>(wlds, R);
    float r[8], i[8], mr[8], mi[8];
    frames_to_spectra<LOGN>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, R, g, tw, lds, wlds, r, i, mr, mi);
    float* mag = reinterpret_cast<float*>(lds);                  // 2 (F/2 + 1) TC <= 5120 (8194) floats of the buffer's 9216 (18432)
    mel_magnitudes_to_lds<LOGN>(mag, g, F, spec.eps, r, i, mr, mi);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    const int live_cols = R.frames - (int)blockIdx.x * g.TC;
    const bool with_log = spec.w_lm != 0.f;                      // an empty filter has M_P = M_T = 0: allowed where the log term is not computed
    mel_filter_sums<NT>(mag, F / 2 + 1, g.TC, LOGN - R.logF, mel_tab(tab, F, nbins), [&](bool owner, int, int c, float mp, float mt) {
        if (owner && c < live_cols) {
            const float d = mt - mp;
            s1 = fmaf(d, d, s1);
            s2 = fmaf(mt, mt, s2);
            if (with_log) s3 += fabsf(logf(mp / mt));
            s4 += fabsf(d);
        }
    });
    s1 = wave_sum_uniform(s1); s2 = wave_sum_uniform(s2); s3 = wave_sum_uniform(s3); s4 = wave_sum_uniform(s4);
    if (lane_id() == 0) { red[wave_id()][0] = s1; red[wave_id()][1] = s2; red[wave_id()][2] = s3; red[wave_id()][3] = s4; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float a = 0.f;
        for (int v = 0; v < NW; ++v) a += red[v][threadIdx.x];
        partials[(((size_t)res * gridDim.y + row) * spec.groups + blockIdx.x) * 4 + threadIdx.x] = a;
    }
}

// dL/dM_P[m][c] goes to LDS behind the magnitudes (dm[m TC + c], n_bins TC <= (F/2 + 1) TC floats: 7680 (8450) of the buffer in all), each
// thread then gathers dL/d|P| of its bins from its at most two filters; the rest is mrstft_bwd_kernel
template <int LOGN, bool LIN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_mel_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, const float* __restrict__ tab,
                      const float* __restrict__ stats, const float* __restrict__ gloss, float* __restrict__ gpred, StftSpec spec, int N, int res,
                      int nbins, int wrt_second) {
    constexpr int NT = ColGeom<LOGN>::T;
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int row = blockIdx.y, F = 1 << R.logF, K = F / 2 + 1;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<NT>(wlds, R);
    float r[8], i[8], mr[8], mi[8];
    frames_to_spectra<LOGN>(pred + (size_t)row * N, target + (size_t)row * N, N, frame, live, R, g, tw, lds, wlds, r, i, mr, mi);
    float* mag = reinterpret_cast<float*>(lds);
    float* dm = mag + 2 * K * g.TC;
    mel_magnitudes_to_lds<LOGN>(mag, g, F, spec.eps, r, i, mr, mi);
    const GradK kk = grad_consts(spec, stats, gloss, res, wrt_second);
    const MelTab t = mel_tab(tab, F, nbins);
    const int TC = g.TC;
    mel_filter_sums<NT>(mag, K, TC, LOGN - R.logF, t, [&](bool owner, int m, int c, float mp, float mt) {
        if (owner) {
            const float sgn = mt > mp ? 1.f : (mt < mp ? -1.f : 0.f);
            float d = kk.sc * (mp - mt) + kk.self * mp;
            if (mp > 0.f) d -= kk.lm * sgn / mp;                 // an empty filter (M_P = 0) reaches no bin
            if constexpr (LIN) d -= kk.lin * sgn;
            dm[m * TC + c] = d;
        }
    });
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q;
        float hr = 0.f, hi = 0.f;
        if (live && k <= F / 2) {
            const Bin b = split_bin(r[q], i[q], mr[q], mi[q]);
            const float praw = b.pr * b.pr + b.pi * b.pi;
            if (!(praw <= spec.eps)) {                           // the clamp has zero slope below eps; a NaN bin goes through
                const f2 w = t.w[k];
                const int ma = t.m0[k], mb = ma + 1 < nbins ? ma + 1 : ma;           // w.y = 0 where filter m0 + 1 does not exist
                const float gm = (w.x * dm[ma * TC + g.c] + w.y * dm[mb * TC + g.c]) / sqrtf(praw);      // dL/d|P| / |P|
                hr = gm * b.pr; hi = gm * b.pi;
            }
        }
        r[q] = hr; i[q] = hi;
    }
    col_fft<1, LOGN>(r, i, g, tw, lds);          // its first exchange starts with a barrier: every dm read above is done by then
    float* grow = gpred + (size_t)row * N;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = g.j + g.T * q;
        const float w = hann_in_frame(n, F, R.win);
        if (live && w != 0.f) atomicAdd(grow + reflect_index(frame * R.hop - F / 2 + n, N), w * r[q]);
    }
}
}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
inline int sl_check() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DASP_OK : (int)e;
}
// log2 of a frame length the transforms take (a power of two in 8..8192), else -1
int fft_log2(int n_fft) {
    int lg = 0;
    while (lg < 30 && (1 << lg) < n_fft) ++lg;
    return (1 << lg) == n_fft && lg >= 3 && lg <= 13 ? lg : -1;
}
bool mel_bins_ok(int n_fft, int n_bins) {
    return fft_log2(n_fft) >= 0 && n_bins >= 1 && n_bins <= MEL_MAXBINS && n_bins <= n_fft / 2 + 1;
}
// the workgroups of resolution r: frame groups x rows (items of the sum / difference loss)
dim3 res_grid(const StftSpec& s, int r, int rows) {
    const int TC = frames_per_group(s.r[r].logF);
    return dim3((unsigned)((s.r[r].frames + TC - 1) / TC), (unsigned)rows);
}
// n_bins: 0 for linear bins, else the mel filters of every resolution
bool stft_spec(int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc, float w_lm, float w_lin, int n_bins,
               StftSpec* out) {
    if (nres <= 0 || nres > SL_MAXRES || !fft || !hop || !win) return false;
    if (!std::isfinite(w_sc) || !std::isfinite(w_lm) || !std::isfinite(w_lin)) return false;
    StftSpec s = {};
    s.nres = nres; s.eps = eps; s.groups = 0; s.w_sc = w_sc; s.w_lm = w_lm; s.w_lin = w_lin;
    for (int r = 0; r < nres; ++r) {
        const int lg = fft_log2(fft[r]);
        if (lg < 0 || hop[r] <= 0 || win[r] <= 0 || win[r] > fft[r] || fft[r] / 2 >= N) return false;
        if (n_bins != 0 && !mel_bins_ok(fft[r], n_bins)) return false;
        s.r[r] = StftRes{lg, hop[r], win[r], 1 + N / hop[r]};
        const int ng = (int)res_grid(s, r, 1).x;
        if (ng > s.groups) s.groups = ng;
    }
    *out = s;
    return true;
}
// tab: the resolution's mel table, or null for linear bins. 512 / 1024 / 2048-point frames on linear bins: 1 / 2 / 4 waves per frame;
// 8192 points: 16 waves; anything else: col_fft
void mrstft_fwd_launch(const float* pred, const float* target, const void* tw, const float* tab, float* partials, const StftSpec& s, int rows,
                       int N, int r, int n_bins, hipStream_t st) {
    const dim3 grid = res_grid(s, r, rows);
    const int lg = s.r[r].logF;
    if (tab) {
        if (lg == 13) hipLaunchKernelGGL(mrstft_mel_fwd_kernel<13>, grid, dim3(1024), 0, st, pred, target, (const f2*)tw, tab, partials, s, N, r, n_bins);
        else hipLaunchKernelGGL(mrstft_mel_fwd_kernel<12>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, tab, partials, s, N, r, n_bins);
        return;
    }
    switch (lg) {
        case 9: hipLaunchKernelGGL(mrstft_fwd_split_kernel<1>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, partials, s, N, r); break;
        case 10: hipLaunchKernelGGL(mrstft_fwd_split_kernel<2>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, partials, s, N, r); break;
        case 11: hipLaunchKernelGGL(mrstft_fwd_split_kernel<4>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, partials, s, N, r); break;
        case 13: hipLaunchKernelGGL(mrstft_fwd_kernel<13>, grid, dim3(1024), 0, st, pred, target, (const f2*)tw, partials, s, N, r); break;
        default: hipLaunchKernelGGL(mrstft_fwd_kernel<12>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, partials, s, N, r);
    }
}
template <bool LIN>
void mrstft_bwd_launch(const float* first, const float* second, const void* tw, const float* tab, const float* stats, const float* gloss,
                       float* gfirst, const StftSpec& s, int rows, int N, int r, int n_bins, int wrt_second, hipStream_t st) {
    const dim3 grid = res_grid(s, r, rows);
    const int lg = s.r[r].logF;
    if (tab) {
        if (lg == 13) hipLaunchKernelGGL((mrstft_mel_bwd_kernel<13, LIN>), grid, dim3(1024), 0, st, first, second, (const f2*)tw, tab, stats, gloss, gfirst, s, N, r, n_bins, wrt_second);
        else hipLaunchKernelGGL((mrstft_mel_bwd_kernel<12, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, tab, stats, gloss, gfirst, s, N, r, n_bins, wrt_second);
        return;
    }
    switch (lg) {
        case 9: hipLaunchKernelGGL((mrstft_bwd_split_kernel<1, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second); break;
        case 10: hipLaunchKernelGGL((mrstft_bwd_split_kernel<2, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second); break;
        case 11: hipLaunchKernelGGL((mrstft_bwd_split_kernel<4, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second); break;
        case 13: hipLaunchKernelGGL((mrstft_bwd_kernel<13, LIN>), grid, dim3(1024), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second); break;
        default: hipLaunchKernelGGL((mrstft_bwd_kernel<12, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second);
    }
}
}  // namespace

extern "C" {

/* tw: 4096 complex (8192 floats), the twiddle table the transforms read */
int dasp_mrstft_table(void* tw, void* stream) {
    if (!tw) return DASP_ERR_ARG;
    hipLaunchKernelGGL(stft_twiddle_kernel, dim3(FFT_N / 256), dim3(256), 0, (hipStream_t)stream, (f2*)tw);
    return sl_check();
}

static int fir_same_launch(const float* a, const float* b, float* ya, float* yb, const float* taps, int ntaps, int rows, int N, int flip,
                           void* stream) {
    if (!a || !ya || !taps || (!b) != (!yb) || rows <= 0 || N <= 0) return DASP_ERR_ARG;
    if (ntaps <= 0 || ntaps > FIR_MAXTAPS || !(ntaps & 1) || rows > 65535) return DASP_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((N + FIR_TILE - 1) / FIR_TILE), (unsigned)rows, b ? 2u : 1u);
    hipLaunchKernelGGL(fir_same_kernel, grid, dim3(FIR_NT), 0, (hipStream_t)stream, a, b, ya, yb, taps, ntaps, flip, N);
    return sl_check();
}
int dasp_fir_same_forward(const float* x0, const float* x1, float* y0, float* y1, const float* taps, int ntaps, int rows, int N, void* stream) {
    return fir_same_launch(x0, x1, y0, y1, taps, ntaps, rows, N, 0, stream);
}
int dasp_fir_same_adjoint(const float* g0, const float* g1, float* gx0, float* gx1, const float* taps, int ntaps, int rows, int N, void* stream) {
    return fir_same_launch(g0, g1, gx0, gx1, taps, ntaps, rows, N, 1, stream);
}
int dasp_fir_taps_store(float* dst, const float* host_taps, int ntaps, void* stream) {
    if (!dst || !host_taps) return DASP_ERR_ARG;
    if (ntaps <= 0 || ntaps > FIR_MAXTAPS) return DASP_ERR_UNSUPPORTED;
    FirTaps t = {};
    for (int k = 0; k < ntaps; ++k) t.h[k] = host_taps[k];
    t.n = ntaps;
    hipLaunchKernelGGL(fir_taps_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, dst, t);
    return sl_check();
}

/* ---- scale="mel" ---- */
/* floats of one resolution's mel table; -1: n_fft not a power of two in 8..8192, or n_bins outside 1..min(256, n_fft / 2 + 1) */
long dasp_mel_table_floats(int n_fft, int n_bins) {
    return mel_bins_ok(n_fft, n_bins) ? mel_table_len(n_fft, n_bins) : -1;
}
/* host_edges: the n_bins + 2 edge frequencies in Hz (fp64, increasing, the first >= 0); they travel as kernel arguments */
int dasp_mel_table_store(float* table, const double* host_edges, double sample_rate, int n_fft, int n_bins, void* stream) {
    if (!table || !host_edges) return DASP_ERR_ARG;
    if (!mel_bins_ok(n_fft, n_bins)) return DASP_ERR_UNSUPPORTED;
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate) || !(host_edges[0] >= 0.0)) return DASP_ERR_ARG;
    MelEdges E = {};
    for (int n = 0; n < n_bins + 2; ++n) {
        if (!std::isfinite(host_edges[n]) || (n > 0 && !(host_edges[n] > host_edges[n - 1]))) return DASP_ERR_ARG;
        E.e[n] = host_edges[n];
    }
    const int K = n_fft / 2 + 1;
    hipLaunchKernelGGL(mel_table_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, E, sample_rate, n_fft, n_bins);
    return sl_check();
}
/* dense: (n_bins, n_fft / 2 + 1) floats, the matrix the table stands for */
int dasp_mel_table_dense(const float* table, float* dense, int n_fft, int n_bins, void* stream) {
    if (!table || !dense) return DASP_ERR_ARG;
    if (!mel_bins_ok(n_fft, n_bins)) return DASP_ERR_UNSUPPORTED;
    const int K = n_fft / 2 + 1;
    hipLaunchKernelGGL(mel_dense_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)n_bins), dim3(256), 0, (hipStream_t)stream, table, dense, n_fft, n_bins);
    return sl_check();
}

}  // extern "C"

// ================================================================================================
// Sum / difference loss of a stereo pair (auraloss.freq.SumAndDifferenceSTFTLoss): the loss above on s = L + R and on d = L - R, as two
// separate losses (each with its own sums, spectral-convergence ratio and means over its `items` rows), from one launch per
// resolution over the (items, 2, N) signals. A workgroup owns a frame group of one batch ITEM - both channels - on the col_fft geometry (every power of two
// 8 .. 8192; frames of 512 / 1024 / 2048 points run here too, there are no split variants): the frame slots of L and R of both signals are
// gathered once per half (4 loads per slot each time, the second time from lines the first brought into the cache - sd_gather_half says
// why not once), (pL + pR) + i (tL + tR) and (pL - pR) + i (tL - tR) are transformed one after the other and reduced to
// the four sums of their half:  partials[(((half * nres + res) * items + item) * groups + group) * 4 + c], stats[(half * nres + res) * 4 + c],
// loss[half]; half 0 = sum, 1 = difference. Fixed summation order throughout: the forward is bit-identical run to run.
// Backward: both halves' one-sided gradient spectra H_s, H_d (grad_consts / grad_bin with the half's own stats and its own element of the
// two-element gloss) go back to channels in the frequency domain, H_L = H_s + H_d, H_R = H_s - H_d, and through ONE packed inverse
// transform: with G_X the Hermitian spectrum of the real frame g_X = Re sum_{k <= F/2} H_X[k] e^{+2 pi i k n / F},
//   G_X[k] = H_X[k] / 2 (0 < k < F/2),  Re H_X[k] (k = 0, F/2),  conj(H_X[F - k]) / 2 (k > F/2),
// Z = G_L + i G_R gives Re IFFT(Z) = g_L and Im IFFT(Z) = g_R: three transforms per item and frame group where two calls of the mono loss
// run four, and one float atomic per sample, frame and channel. After frames_to_spectra's exchange a thread holds Z[k] AND Z[F - k] for
// each of its slots k = j + T q over the whole range 0 .. F - 1, so the thread that owns an upper slot k > F/2 forms bin F - k itself from the
// swapped pair: no further exchange; the price is grad_bin on F instead of F/2 + 1 bins.
namespace dasp {

// One half only (DIFF: L - R, else L + R); every kernel gathers twice, once per half. Gathering both halves at once (4 loads per slot in
// all) holds the second half's 16 registers through the first half's transform: 128 .. 145 VGPRs, scratch spills in the 8192-point
// instances and one 512-thread workgroup per CU where the mono kernels run three - measured at twice the mono kernels' time per transform.
// The second gather reads lines the first one brought in.
template <bool DIFF>
__device__ __forceinline__ void sd_gather_half(const float* __restrict__ aL, const float* __restrict__ aR, const float* __restrict__ bL,
                                               const float* __restrict__ bR, int N, int frame, bool live, const StftRes& R, const ColCfg& g,
                                               const float* wlds, float (&r)[8], float (&i)[8]) {
    const int F = 1 << R.logF;
    float ar[8], br[8];
    int s[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        s[q] = reflect_index(frame * R.hop - F / 2 + g.j + g.T * q, N);
        s[q] = s[q] < 0 ? 0 : (s[q] >= N ? N - 1 : s[q]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { r[q] = aL[s[q]]; ar[q] = aR[s[q]]; }
#pragma unroll
    for (int q = 0; q < 8; ++q) { i[q] = bL[s[q]]; br[q] = bR[s[q]]; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float w = live ? wlds[g.j + g.T * q] : 0.f;
        r[q] = w * (DIFF ? r[q] - ar[q] : r[q] + ar[q]);
        i[q] = w * (DIFF ? i[q] - br[q] : i[q] + br[q]);
    }
}
// The thread's coordinates for the next phase of a kernel (second half, inverse transform), behind an empty dependency on two results (a, b)
// of the phase before: the copy of (j, c) and of the frame index is opaque to the compiler, so the next phase's loads cannot be hoisted
// above the phase before, and its twiddles, LDS addresses and sample indices - common subexpressions of the earlier phase's - are formed
// again instead of being held in registers across both (that alone is 20 .. 30 VGPRs, the difference between two and three workgroups per
// CU). No instruction is emitted. tests/test_sumdiff_stft_cpu.py holds the built kernels to their register counts and to zero scratch.
__device__ __forceinline__ ColCfg sd_next_phase(const ColCfg& g, int& frame, float a, float b) {
    ColCfg o = g;
    asm volatile("" : "+v"(frame), "+v"(o.j), "+v"(o.c) : "v"(a), "v"(b));
    return o;
}
// frames_to_spectra behind its gather: r/i <- Z[j + T q], mr/mi <- Z[F - (j + T q)]
template <int LOGN>
__device__ __forceinline__ void regs_to_spectra(const StftRes& R, const ColCfg& g, const f2* __restrict__ tw, f2* lds, float (&r)[8], float (&i)[8],
                                                float (&mr)[8], float (&mi)[8]) {
    const int F = 1 << R.logF;
    col_fft<-1, LOGN>(r, i, g, tw, lds);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) lds[fft_pad(g.j + g.T * q) * g.TC + g.c] = f2{r[q], i[q]};
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f2 m = lds[fft_pad((F - (g.j + g.T * q)) & (F - 1)) * g.TC + g.c];
        mr[q] = m.x; mi[q] = m.y;
    }
    __syncthreads();
}
// the eight sums of a workgroup (4 per half) -> its partials
template <int NW>
__device__ __forceinline__ void sd_write_partials(float (&s)[8], float (*red)[8], float* __restrict__ partials, const StftSpec& spec, int res) {
#pragma unroll
    for (int c = 0; c < 8; ++c) s[c] = wave_sum_uniform(s[c]);
    if (lane_id() == 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) red[wave_id()][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        float a = 0.f;
        for (int v = 0; v < NW; ++v) a += red[v][threadIdx.x];
        const int half = threadIdx.x >> 2, c = threadIdx.x & 3;
        partials[((((size_t)half * spec.nres + res) * gridDim.y + blockIdx.y) * spec.groups + blockIdx.x) * 4 + c] = a;
    }
}

template <int LOGN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T, LOGN == 13 ? 4 : 6)
mrstft_sd_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, float* __restrict__ partials,
                     StftSpec spec, int N, int res) {
    constexpr int NT = ColGeom<LOGN>::T, NW = NT / 64;
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    __shared__ float red[NW][8];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int item = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<NT>(wlds, R);
    const float* pL = pred + (size_t)(2 * item) * N;
    const float* tL = target + (size_t)(2 * item) * N;
    float r[8], i[8], mr[8], mi[8];
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    sd_gather_half<false>(pL, pL + N, tL, tL + N, N, frame, live, R, g, wlds, r, i);
    regs_to_spectra<LOGN>(R, g, tw, lds, r, i, mr, mi);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (live && g.j + g.T * q <= F / 2) loss_terms(split_bin(r[q], i[q], mr[q], mi[q]), spec.eps, s[0], s[1], s[2], s[3]);
    int frame2 = frame;
    const ColCfg g2 = sd_next_phase(g, frame2, s[0], s[2]);
    sd_gather_half<true>(pL, pL + N, tL, tL + N, N, frame2, live, R, g2, wlds, r, i);
    regs_to_spectra<LOGN>(R, g2, tw, lds, r, i, mr, mi);
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (live && g2.j + g2.T * q <= F / 2) loss_terms(split_bin(r[q], i[q], mr[q], mi[q]), spec.eps, s[4], s[5], s[6], s[7]);
    sd_write_partials<NW>(s, red, partials, spec, res);
}

// slot k of the Hermitian spectrum G from the one-sided gradient bin H of bin k (k <= F/2) or F - k (k > F/2)
__device__ __forceinline__ void sd_hermitian_slot(int k, int F, float hr, float hi, float& gr, float& gi) {
    const bool edge = k == 0 || k == F / 2;
    gr = edge ? hr : 0.5f * hr;
    gi = edge ? 0.f : (k > F / 2 ? -0.5f * hi : 0.5f * hi);
}
// r/i (Z[k]), mr/mi (Z[F - k]) of one half -> r/i = G[k] of that half's gradient frame
template <bool LIN>
__device__ __forceinline__ void sd_grad_spectrum(const ColCfg& g, int F, bool live, float eps, const GradK& kk, float (&r)[8], float (&i)[8],
                                                 const float (&mr)[8], const float (&mi)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q;
        const Bin b = k > F / 2 ? split_bin(mr[q], mi[q], r[q], i[q]) : split_bin(r[q], i[q], mr[q], mi[q]);
        float hr = 0.f, hi = 0.f;
        if (live) grad_bin<LIN>(b, eps, kk, hr, hi);
        sd_hermitian_slot(k, F, hr, hi, r[q], i[q]);
    }
}
// Z = G_L + i G_R from the two halves' G (G_L = G_s + G_d, G_R = G_s - G_d), the packed inverse transform, and the two scatters
template <int LOGN>
__device__ __forceinline__ void sd_inverse_and_scatter(float (&r)[8], float (&i)[8], const float (&dr)[8], const float (&di)[8], const StftRes& R,
                                                       const ColCfg& g, const f2* __restrict__ tw, f2* lds, int frame, bool live, int N,
                                                       float* __restrict__ gL, float* __restrict__ gR) {
    const int F = 1 << R.logF;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float lr = r[q] + dr[q], li = i[q] + di[q], rr = r[q] - dr[q], ri = i[q] - di[q];
        r[q] = lr - ri; i[q] = li + rr;
    }
    col_fft<1, LOGN>(r, i, g, tw, lds);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = g.j + g.T * q;
        const float w = hann_in_frame(n, F, R.win);
        if (live && w != 0.f) {
            const int s = reflect_index(frame * R.hop - F / 2 + n, N);
            atomicAdd(gL + s, w * r[q]);
            atomicAdd(gR + s, w * i[q]);
        }
    }
}

// gfirst (2 items, N) must be zero on entry; gloss: two device floats, d(objective)/d(sum_loss) and d(objective)/d(diff_loss)
template <int LOGN, bool LIN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_sd_bwd_kernel(const float* __restrict__ first, const float* __restrict__ second, const f2* __restrict__ tw, const float* __restrict__ stats,
                     const float* __restrict__ gloss, float* __restrict__ gfirst, StftSpec spec, int N, int res, int wrt_second) {
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int item = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<ColGeom<LOGN>::T>(wlds, R);
    const float* aL = first + (size_t)(2 * item) * N;
    const float* bL = second + (size_t)(2 * item) * N;
    float r[8], i[8], dr[8], di[8], mr[8], mi[8];
    sd_gather_half<false>(aL, aL + N, bL, bL + N, N, frame, live, R, g, wlds, r, i);
    regs_to_spectra<LOGN>(R, g, tw, lds, r, i, mr, mi);
    sd_grad_spectrum<LIN>(g, F, live, spec.eps, grad_consts(spec, stats, gloss, res, wrt_second), r, i, mr, mi);
    int frame2 = frame;
    const ColCfg g2 = sd_next_phase(g, frame2, r[0], i[0]);
    sd_gather_half<true>(aL, aL + N, bL, bL + N, N, frame2, live, R, g2, wlds, dr, di);
    regs_to_spectra<LOGN>(R, g2, tw, lds, dr, di, mr, mi);
    sd_grad_spectrum<LIN>(g2, F, live, spec.eps, grad_consts(spec, stats + 4 * spec.nres, gloss + 1, res, wrt_second), dr, di, mr, mi);
    const ColCfg g3 = sd_next_phase(g, frame2, dr[0], di[0]);
    float* gL = gfirst + (size_t)(2 * item) * N;
    sd_inverse_and_scatter<LOGN>(r, i, dr, di, R, g3, tw, lds, frame2, live, N, gL, gL + N);
}

// ---- mel-scaled magnitudes: mrstft_mel_fwd_kernel / mrstft_mel_bwd_kernel's steps once per half, on the same per-resolution tables ----
template <int LOGN>
__device__ __forceinline__ void sd_mel_half_sums(float* mag, const ColCfg& g, const StftRes& R, const StftSpec& spec, const MelTab& t, int live_cols,
                                                 const float (&r)[8], const float (&i)[8], const float (&mr)[8], const float (&mi)[8],
                                                 float& s1, float& s2, float& s3, float& s4) {
    const int F = 1 << R.logF;
    mel_magnitudes_to_lds<LOGN>(mag, g, F, spec.eps, r, i, mr, mi);
    const bool with_log = spec.w_lm != 0.f;
    mel_filter_sums<ColGeom<LOGN>::T>(mag, F / 2 + 1, g.TC, LOGN - R.logF, t, [&](bool owner, int, int c, float mp, float mt) {
        if (owner && c < live_cols) {
            const float d = mt - mp;
            s1 = fmaf(d, d, s1);
            s2 = fmaf(mt, mt, s2);
            if (with_log) s3 += fabsf(logf(mp / mt));
            s4 += fabsf(d);
        }
    });
    __syncthreads();             // the magnitudes are read: the buffer goes back to the next transform
}

template <int LOGN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T, LOGN == 13 ? 4 : 6)
mrstft_sd_mel_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const f2* __restrict__ tw, const float* __restrict__ tab,
                         float* __restrict__ partials, StftSpec spec, int N, int res, int nbins) {
    constexpr int NT = ColGeom<LOGN>::T, NW = NT / 64;
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    __shared__ float red[NW][8];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int item = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<NT>(wlds, R);
    const float* pL = pred + (size_t)(2 * item) * N;
    const float* tL = target + (size_t)(2 * item) * N;
    float r[8], i[8], mr[8], mi[8];
    float* mag = reinterpret_cast<float*>(lds);
    const MelTab t = mel_tab(tab, F, nbins);
    const int live_cols = R.frames - (int)blockIdx.x * g.TC;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    sd_gather_half<false>(pL, pL + N, tL, tL + N, N, frame, live, R, g, wlds, r, i);
    regs_to_spectra<LOGN>(R, g, tw, lds, r, i, mr, mi);
    sd_mel_half_sums<LOGN>(mag, g, R, spec, t, live_cols, r, i, mr, mi, s[0], s[1], s[2], s[3]);
    int frame2 = frame;
    const ColCfg g2 = sd_next_phase(g, frame2, s[0], s[2]);
    sd_gather_half<true>(pL, pL + N, tL, tL + N, N, frame2, live, R, g2, wlds, r, i);
    regs_to_spectra<LOGN>(R, g2, tw, lds, r, i, mr, mi);
    sd_mel_half_sums<LOGN>(mag, g2, R, spec, t, live_cols, r, i, mr, mi, s[4], s[5], s[6], s[7]);
    sd_write_partials<NW>(s, red, partials, spec, res);
}

// one half: magnitudes and dL/dM_P to LDS (mrstft_mel_bwd_kernel), then r/i = G[k]: every slot gathers dL/d|P| of its bin (k, or F - k for
// an upper slot) from that bin's at most two filters
template <int LOGN, bool LIN>
__device__ __forceinline__ void sd_mel_grad_spectrum(float* mag, const ColCfg& g, const StftRes& R, const StftSpec& spec, const MelTab& t,
                                                     const GradK& kk, bool live, float (&r)[8], float (&i)[8], const float (&mr)[8],
                                                     const float (&mi)[8]) {
    const int F = 1 << R.logF, K = F / 2 + 1, TC = g.TC;
    float* dm = mag + 2 * K * TC;
    mel_magnitudes_to_lds<LOGN>(mag, g, F, spec.eps, r, i, mr, mi);
    mel_filter_sums<ColGeom<LOGN>::T>(mag, K, TC, LOGN - R.logF, t, [&](bool owner, int m, int c, float mp, float mt) {
        if (owner) {
            const float sgn = mt > mp ? 1.f : (mt < mp ? -1.f : 0.f);
            float d = kk.sc * (mp - mt) + kk.self * mp;
            if (mp > 0.f) d -= kk.lm * sgn / mp;
            if constexpr (LIN) d -= kk.lin * sgn;
            dm[m * TC + c] = d;
        }
    });
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = g.j + g.T * q, kb = k > F / 2 ? F - k : k;
        const Bin b = k > F / 2 ? split_bin(mr[q], mi[q], r[q], i[q]) : split_bin(r[q], i[q], mr[q], mi[q]);
        float hr = 0.f, hi = 0.f;
        const float praw = b.pr * b.pr + b.pi * b.pi;
        if (live && !(praw <= spec.eps)) {
            const f2 w = t.w[kb];
            const int ma = t.m0[kb], mb = ma + 1 < t.B ? ma + 1 : ma;
            const float gm = (w.x * dm[ma * TC + g.c] + w.y * dm[mb * TC + g.c]) / sqrtf(praw);
            hr = gm * b.pr; hi = gm * b.pi;
        }
        sd_hermitian_slot(k, F, hr, hi, r[q], i[q]);
    }
    __syncthreads();             // dm is read: the buffer goes back to the next transform
}

template <int LOGN, bool LIN>
__global__ void __launch_bounds__(ColGeom<LOGN>::T)
mrstft_sd_mel_bwd_kernel(const float* __restrict__ first, const float* __restrict__ second, const f2* __restrict__ tw, const float* __restrict__ tab,
                         const float* __restrict__ stats, const float* __restrict__ gloss, float* __restrict__ gfirst, StftSpec spec, int N, int res,
                         int nbins, int wrt_second) {
    __shared__ f2 lds[ColGeom<LOGN>::LDS];
    __shared__ float wlds[1 << LOGN];
    StftRes R = spec.r[res];
    if constexpr (LOGN == 13) R.logF = 13;
    const ColCfg g = col_config<LOGN>(R.logF, threadIdx.x);
    const int item = blockIdx.y, F = 1 << R.logF;
    if ((int)blockIdx.x * g.TC >= R.frames) return;
    const int frame = blockIdx.x * g.TC + g.c;
    const bool live = frame < R.frames;
    window_to_lds<ColGeom<LOGN>::T>(wlds, R);
    const float* aL = first + (size_t)(2 * item) * N;
    const float* bL = second + (size_t)(2 * item) * N;
    float r[8], i[8], dr[8], di[8], mr[8], mi[8];
    sd_gather_half<false>(aL, aL + N, bL, bL + N, N, frame, live, R, g, wlds, r, i);
    float* mag = reinterpret_cast<float*>(lds);
    const MelTab t = mel_tab(tab, F, nbins);
    regs_to_spectra<LOGN>(R, g, tw, lds, r, i, mr, mi);
    sd_mel_grad_spectrum<LOGN, LIN>(mag, g, R, spec, t, grad_consts(spec, stats, gloss, res, wrt_second), live, r, i, mr, mi);
    int frame2 = frame;
    const ColCfg g2 = sd_next_phase(g, frame2, r[0], i[0]);
    sd_gather_half<true>(aL, aL + N, bL, bL + N, N, frame2, live, R, g2, wlds, dr, di);
    regs_to_spectra<LOGN>(R, g2, tw, lds, dr, di, mr, mi);
    sd_mel_grad_spectrum<LOGN, LIN>(mag, g2, R, spec, t, grad_consts(spec, stats + 4 * spec.nres, gloss + 1, res, wrt_second), live, dr, di, mr, mi);
    const ColCfg g3 = sd_next_phase(g, frame2, dr[0], di[0]);
    float* gL = gfirst + (size_t)(2 * item) * N;
    sd_inverse_and_scatter<LOGN>(r, i, dr, di, R, g3, tw, lds, frame2, live, N, gL, gL + N);
}
}  // namespace dasp

namespace {
template <bool LIN>
void mrstft_sd_bwd_launch(const float* first, const float* second, const void* tw, const float* tab, const float* stats, const float* gloss,
                          float* gfirst, const StftSpec& s, int items, int N, int r, int n_bins, int wrt_second, hipStream_t st) {
    const dim3 grid = res_grid(s, r, items);
    const bool big = s.r[r].logF == 13;
    if (tab) {
        if (big) hipLaunchKernelGGL((mrstft_sd_mel_bwd_kernel<13, LIN>), grid, dim3(1024), 0, st, first, second, (const f2*)tw, tab, stats, gloss, gfirst, s, N, r, n_bins, wrt_second);
        else hipLaunchKernelGGL((mrstft_sd_mel_bwd_kernel<12, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, tab, stats, gloss, gfirst, s, N, r, n_bins, wrt_second);
    } else {
        if (big) hipLaunchKernelGGL((mrstft_sd_bwd_kernel<13, LIN>), grid, dim3(1024), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second);
        else hipLaunchKernelGGL((mrstft_sd_bwd_kernel<12, LIN>), grid, dim3(512), 0, st, first, second, (const f2*)tw, stats, gloss, gfirst, s, N, r, wrt_second);
    }
}
void mrstft_sd_fwd_launch(const float* pred, const float* target, const void* tw, const float* tab, float* partials, const StftSpec& s, int items,
                          int N, int r, int n_bins, hipStream_t st) {
    const dim3 grid = res_grid(s, r, items);
    const bool big = s.r[r].logF == 13;
    if (tab) {
        if (big) hipLaunchKernelGGL(mrstft_sd_mel_fwd_kernel<13>, grid, dim3(1024), 0, st, pred, target, (const f2*)tw, tab, partials, s, N, r, n_bins);
        else hipLaunchKernelGGL(mrstft_sd_mel_fwd_kernel<12>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, tab, partials, s, N, r, n_bins);
    } else {
        if (big) hipLaunchKernelGGL(mrstft_sd_fwd_kernel<13>, grid, dim3(1024), 0, st, pred, target, (const f2*)tw, partials, s, N, r);
        else hipLaunchKernelGGL(mrstft_sd_fwd_kernel<12>, grid, dim3(512), 0, st, pred, target, (const f2*)tw, partials, s, N, r);
    }
}
// The two layouts of the loss share everything but the kernels of a resolution: halves = 1, the mono loss on `rows` signals; halves = 2, the
// sum / difference loss on `rows` items of two channel rows each. n_bins and mel_tables: both zero (linear bins) or both set (mel).
long partial_floats(int halves, long rows, int N, int nres, const int* fft, const int* hop, const int* win, int n_bins) {
    StftSpec s;
    if (!stft_spec(N, nres, fft, hop, win, 0.f, 1.f, 1.f, 0.f, n_bins, &s)) return -1;
    return (long)halves * nres * rows * s.groups * 4;
}
// the checks of both directions, in the order of their statuses; io: the direction's own three buffers
int stft_check(const float* pred, const float* target, const void* tw, const void* const* mel_tables, const void* io0, const void* io1,
               const void* io2, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc, float w_lm,
               float w_lin, int n_bins, StftSpec* s) {
    if (!pred || !target || !tw || !io0 || !io1 || !io2 || rows <= 0 || N <= 0 || (n_bins != 0) != (mel_tables != nullptr)) return DASP_ERR_ARG;
    if (!stft_spec(N, nres, fft, hop, win, eps, w_sc, w_lm, w_lin, n_bins, s) || rows > 65535) return DASP_ERR_UNSUPPORTED;
    for (int r = 0; mel_tables && r < nres; ++r)
        if (!mel_tables[r]) return DASP_ERR_ARG;
    return DASP_OK;
}
int stft_forward(int halves, const float* pred, const float* target, const void* tw, const void* const* mel_tables, float* partials, float* stats,
                 float* loss, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc, float w_lm,
                 float w_lin, int n_bins, void* stream) {
    StftSpec s;
    const int bad = stft_check(pred, target, tw, mel_tables, partials, stats, loss, rows, N, nres, fft, hop, win, eps, w_sc, w_lm, w_lin, n_bins, &s);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    for (int r = 0; r < nres; ++r) {
        const float* tab = mel_tables ? (const float*)mel_tables[r] : nullptr;
        if (halves == 2) mrstft_sd_fwd_launch(pred, target, tw, tab, partials, s, rows, N, r, n_bins, st);
        else mrstft_fwd_launch(pred, target, tw, tab, partials, s, rows, N, r, n_bins, st);
    }
    hipLaunchKernelGGL(mrstft_reduce_kernel, dim3((unsigned)(halves * nres * 4)), dim3(1024), 0, st, (const float*)partials, s, rows, stats);
    hipLaunchKernelGGL(mrstft_finalize_kernel, dim3(1), dim3(64), 0, st, s, rows, n_bins, halves, stats, loss);
    return sl_check();
}
// wrt_target: the same kernels with the two signals swapped (grad_bin)
int stft_backward(int halves, const float* pred, const float* target, const void* tw, const void* const* mel_tables, const float* stats,
                  const float* gloss, float* grad, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc,
                  float w_lm, float w_lin, int n_bins, int wrt_target, void* stream) {
    if (wrt_target != 0 && wrt_target != 1) return DASP_ERR_ARG;
    StftSpec s;
    const int bad = stft_check(pred, target, tw, mel_tables, stats, gloss, grad, rows, N, nres, fft, hop, win, eps, w_sc, w_lm, w_lin, n_bins, &s);
    if (bad) return bad;
    const float* first = wrt_target ? target : pred;
    const float* second = wrt_target ? pred : target;
    hipStream_t st = (hipStream_t)stream;
    if (zero_async(grad, (size_t)halves * rows * N * sizeof(float), st) != hipSuccess) return sl_check();
    for (int r = 0; r < nres; ++r) {
        const float* tab = mel_tables ? (const float*)mel_tables[r] : nullptr;
        const bool lin = s.w_lin != 0.f;
        if (halves == 2) (lin ? mrstft_sd_bwd_launch<true> : mrstft_sd_bwd_launch<false>)(first, second, tw, tab, stats, gloss, grad, s, rows, N, r, n_bins, wrt_target, st);
        else (lin ? mrstft_bwd_launch<true> : mrstft_bwd_launch<false>)(first, second, tw, tab, stats, gloss, grad, s, rows, N, r, n_bins, wrt_target, st);
    }
    return sl_check();
}
}  // namespace

extern "C" {

/* floats of `partials` for rows signals of N samples; -1 if the resolutions are not supported (n_fft a power of two in 8..8192,
 * win <= n_fft, n_fft / 2 < N, at most 8 resolutions; n_bins 0, or 1..min(256, n_fft / 2 + 1) mel filters) */
long dasp_mrstft_partial_floats(long rows, int N, int nres, const int* fft, const int* hop, const int* win, int n_bins) {
    return partial_floats(1, rows, N, nres, fft, hop, win, n_bins);
}
/* pred, target (rows, N); stats (4 * nres floats, kept for the backward); loss: 1 float. mel_tables: null with n_bins = 0 (linear bins), or
 * nres device pointers (a host array), table r built by dasp_mel_table_store for fft[r] and n_bins */
int dasp_mrstft_forward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, float* partials, float* stats,
                        float* loss, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc,
                        float w_log_mag, float w_lin_mag, int n_bins, void* stream) {
    return stft_forward(1, pred, target, tw, mel_tables, partials, stats, loss, rows, N, nres, fft, hop, win, eps, w_sc, w_log_mag, w_lin_mag, n_bins,
                        stream);
}
/* grad (rows, N) is overwritten with gloss * d loss / d pred (gloss: device scalar), or with wrt_target = 1 gloss * d loss / d target
 * (auraloss differentiates both arguments: a consistency loss between two model outputs needs it; the reference's call sites pass the
 * reference signal there and never ask) */
int dasp_mrstft_backward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, const float* stats,
                         const float* gloss, float* grad, int rows, int N, int nres, const int* fft, const int* hop, const int* win, float eps,
                         float w_sc, float w_log_mag, float w_lin_mag, int n_bins, int wrt_target, void* stream) {
    return stft_backward(1, pred, target, tw, mel_tables, stats, gloss, grad, rows, N, nres, fft, hop, win, eps, w_sc, w_log_mag, w_lin_mag, n_bins,
                         wrt_target, stream);
}
/* floats of `partials` for items stereo pairs of N samples: 2 halves x nres x items x groups x 4; -1 as dasp_mrstft_partial_floats */
long dasp_mrstft_sd_partial_floats(long items, int N, int nres, const int* fft, const int* hop, const int* win, int n_bins) {
    return items <= 0 ? -1 : partial_floats(2, items, N, nres, fft, hop, win, n_bins);
}
/* pred, target (items, 2, N); stats: 8 * nres floats (kept for the backward); loss: 2 floats (sum_loss, diff_loss) */
int dasp_mrstft_sd_forward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, float* partials, float* stats,
                           float* loss, int items, int N, int nres, const int* fft, const int* hop, const int* win, float eps, float w_sc,
                           float w_log_mag, float w_lin_mag, int n_bins, void* stream) {
    return stft_forward(2, pred, target, tw, mel_tables, partials, stats, loss, items, N, nres, fft, hop, win, eps, w_sc, w_log_mag, w_lin_mag, n_bins,
                        stream);
}
/* grad (items, 2, N) is overwritten with gloss[0] d sum_loss / d x + gloss[1] d diff_loss / d x, x = pred or (wrt_target = 1) target
 * (gloss: two device floats) */
int dasp_mrstft_sd_backward(const float* pred, const float* target, const void* tw, const void* const* mel_tables, const float* stats,
                            const float* gloss, float* grad, int items, int N, int nres, const int* fft, const int* hop, const int* win, float eps,
                            float w_sc, float w_log_mag, float w_lin_mag, int n_bins, int wrt_target, void* stream) {
    return stft_backward(2, pred, target, tw, mel_tables, stats, gloss, grad, items, N, nres, fft, hop, win, eps, w_sc, w_log_mag, w_lin_mag, n_bins,
                         wrt_target, stream);
}

}  // extern "C"
