// Level metering and normalisation: ITU-R BS.1770-4 integrated loudness (K-weighting, 400 ms blocks with 75 % overlap, absolute and
// relative gates) with its gradient, and per-row peak normalisation.
//
// The K-weighting is a fixed fourth-order filter (two biquads designed from the sample rate alone), so everything that depends on it is
// worked out on the host in fp64 and handed to the kernels BY VALUE in an argument struct: the 4x4 state transition over a lane's chunk
// and its powers (1, 2, 4 ... 64 chunks), the response of each sample of a chunk to the state at the chunk's start, and - for the
// segmented path - the transition over a segment. No device-side tables in global memory (a workgroup copies the powers and the
// response rows into its LDS and reads them as broadcasts: kept in scalar registers they spilled), no host synchronisation, nothing to
// zero: every call is a few plain kernel nodes under graph capture.
//
//   filter pass  one workgroup of 256 lanes owns a (row, segment) and walks it in tiles of 256 chunks x 32 samples. A lane runs its
//                chunk from a zero state; the chunk end states are scanned across the 64 lanes of a wave (Hillis-Steele on the transition
//                powers), the four wave totals cross through LDS, and each lane corrects its samples with the state at its chunk's start.
//                A wave moves its 2048 samples as coalesced 16-byte accesses and transposes them to chunks through an LDS image of its own.
//                The recurrence, the states and the scan are fp64 throughout (the high-pass has a double pole at radius 0.995: an fp32
//                recurrence is not good enough); samples are fp32 in memory and the per-sample state correction is an fp32 dot product.
//                One template over the direction and the epilogue:
//                  forward            -> squares summed into the H-sample sub-blocks (H = 100 ms) they fall in; with STORE also the
//                                        K-weighted signal for the backward pass (4 B written per sample)
//                  backward           <- the saved K-weighted signal times 2 x coverage weight of its sub-block x upstream gradient on
//                                        load, filtered backwards in time, -> gx
//                  state pre-pass     -> the end state of a segment from a zero start (few rows only, either direction)
//                Sub-block sums: per lane fp32 over at most 32 squares (summed again in fp64 where that sum is inf: a sample above
//                1.8e19), then fp64 in a fixed order (a wave tree per sub-block the wave touches, stored per wave; the gate launch adds
//                a row's waves in sequence): bit-identical run to run, no atomics.
//   few rows     a row is cut into segments that run as workgroups of their own: the pre-pass leaves every segment's end state from a zero
//                start, and the main pass begins by chaining the states of the segments before its own (at most 256 4-vectors, one
//                thread) - two launches, and no workgroup ever waits for another one.
//   gate         one workgroup per item: sub-block sums from the waves' partials in a fixed order, block powers from four consecutive sub-blocks,
//                both gates in fp64, L in fp32, and the coverage weights of the backward pass (-0.f throughout for an empty gate: the
//                backward pass then writes exact zeros and reads no sample). The gates are IEEE comparisons: a block whose power is NaN
//                passes neither, so a NaN sample leaves L finite where clean blocks remain, and the row's gradient NaN (NaN x 0 coverage).
//   peak         max |x| with the lowest index attaining it per (row, segment), then a scaling pass; backward: sum g x per (row,
//                segment), then one elementwise pass that adds the correction at the index of the maximum.
// Rows need 4-byte alignment only: samples are moved as 16-byte vectors through a type that claims no more (global dwordx4 needs no more).
#include "common.hpp"

#include <math.h>

using namespace dasp;

namespace {

constexpr int LD_L = 32;                    // samples per lane and tile: spans at most two sub-blocks (H >= 800)
constexpr int LD_NT = 256;                  // lanes per workgroup
constexpr int LD_NW = LD_NT / 64;
constexpr int LD_TILE = LD_NT * LD_L;       // 8192 samples
constexpr int LD_NP = 7;                    // transition powers: 1, 2, 4, 8, 16, 32, 64 chunks
constexpr int LD_PITCH = LD_L + 4;          // floats between the chunks of a wave's LDS image: 16-byte reads of 64 chunks spread over all banks
constexpr int LD_BINS = 4;                  // sub-blocks a wave's 2048 samples can touch: 2047 / 800 + 2
constexpr long LD_FILL = 1024;              // workgroups that fill the chip (256 CUs x 4)
constexpr int LD_MAX_SEG = 256;             // segments per row at most (the chain prologue stages their states in LDS)
constexpr int LD_MAX_CH = 5;
constexpr long LD_MAX_N = 1L << 30;         // in-row indices are 32-bit
constexpr unsigned LD_EMPTY_GATE = 0x80000000u;      // -0.f in a row's coverage weights: no block of the item passed the gates
enum { LD_STATE = 0, LD_SUMS = 1, LD_SUMS_STORE = 2, LD_STORE = 3 };

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));       // 16 bytes at a 4-byte aligned address

struct LdTab {
    double P[LD_NP][16];        // P[k] = M^(32 * 2^k), row-major
    double MS[16];              // M^S: the transition over a full segment
    double c[2][5];             // b0 b1 b2 a1 a2 of the two sections (a0 = 1)
    float R[LD_L][4];           // y[k] += R[k] . (state at the chunk's start)
};

struct LdArgs {
    const float* in;            // x (forward) or the saved K-weighted signal (backward), (rows, N)
    float* out;                 // K-weighted signal (forward, STORE) or gx (backward)
    const float* cov;           // backward: (rows, nsub) coverage weights
    const float* gL;            // backward: (items) upstream gradient
    double* ends;               // (rows, G, 4) segment end states from a zero start
    double* partial;            // forward: (rows, nq, 4) sub-block sums of each wave's 2048 samples (nq waves per row)
    int N, S, G, H, nsub, chs, nq;
};

__device__ __forceinline__ void ld_matvec(const double (&P)[16], const double (&v)[4], double (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fma(P[4 * i + 3], v[3], fma(P[4 * i + 2], v[2], fma(P[4 * i + 1], v[1], P[4 * i] * v[0])));
}

// One sample through both sections (direct form II transposed), fp64.
__device__ __forceinline__ double ld_step(const double (&c)[2][5], double (&s)[4], double x) {
    const double ya = fma(c[0][0], x, s[0]);
    s[0] = fma(c[0][1], x, fma(-c[0][3], ya, s[1]));
    s[1] = fma(c[0][2], x, -c[0][4] * ya);
    const double yb = fma(c[1][0], ya, s[2]);
    s[2] = fma(c[1][1], ya, fma(-c[1][3], yb, s[3]));
    s[3] = fma(c[1][2], ya, -c[1][4] * yb);
    return yb;
}

// BWD: the row is walked from its last sample to its first (logical position m <-> sample N - 1 - m) and the input is weighted on load.
template <bool BWD, int EPI>
__global__ void __launch_bounds__(LD_NT) ld_filter_kernel(const LdArgs a, const LdTab t) {
    __shared__ double tot[2][LD_NW][4];                     // wave totals of a tile, by tile parity
    __shared__ double Pl[LD_NP][16];                        // the transition powers and the response rows, read as LDS broadcasts
    __shared__ __attribute__((aligned(16))) float Rl[EPI == LD_STATE ? 1 : LD_L][4];
    __shared__ __attribute__((aligned(16))) float img[LD_NW][64 * LD_PITCH];      // a wave's 2048 samples, chunks 36 floats apart
    __shared__ double Q[EPI == LD_STATE ? 1 : 16][64];      // Q[.][l] = M^(32 l)
    __shared__ double stage[EPI == LD_STATE ? 1 : LD_MAX_SEG][4];
    __shared__ double start[4];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int gsegs = EPI == LD_STATE ? a.G - 1 : a.G;      // the pre-pass leaves the last segment out
    const long row = (long)blockIdx.x / gsegs;
    const int g = (int)((long)blockIdx.x - row * gsegs);
    const int N = a.N, H = a.H;
    const int mseg = g * a.S;
    const int seglen = N - mseg < a.S ? N - mseg : a.S;
    const int ntiles = (seglen + LD_TILE - 1) / LD_TILE;
    const float* __restrict__ in = a.in + row * N;
    float* __restrict__ out = a.out ? a.out + row * N : nullptr;

    if (BWD && __float_as_uint(a.cov[row * a.nsub]) == LD_EMPTY_GATE) {      // no block past the gates (uniform over the workgroup, no barrier
        if (EPI != LD_STATE)                                                 // before this): L is -inf and the gradient exactly 0, whatever
            for (int i = tid; i < seglen; i += LD_NT) out[N - mseg - seglen + i] = 0.f;      // the samples and the upstream gradient hold
        return;
    }
    double c[4] = {0.0, 0.0, 0.0, 0.0};                     // state at the start of the tile
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < LD_NP; ++k)
#pragma unroll
            for (int i = 0; i < 16; ++i) Pl[k][i] = t.P[k][i];
        if (EPI != LD_STATE) {
#pragma unroll
            for (int k = 0; k < LD_L; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) Rl[k][i] = t.R[k][i];
        }
    }
    if (EPI == LD_STATE) __syncthreads();
    if (EPI != LD_STATE) {
        if (tid < 64) {                                      // M^(32 lane) from the powers of two
            double q[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) q[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (lane & (1 << k)) {
                    double r[16];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            r[4 * i + j] = fma(t.P[k][4 * i + 3], q[12 + j], fma(t.P[k][4 * i + 2], q[8 + j], fma(t.P[k][4 * i + 1], q[4 + j], t.P[k][4 * i] * q[j])));
#pragma unroll
                    for (int i = 0; i < 16; ++i) q[i] = r[i];
                }
#pragma unroll
            for (int i = 0; i < 16; ++i) Q[i][lane] = q[i];
        }
        if (g > 0) {                                         // the chain step: states of the segments before this one, in sequence
            for (int q = tid; q < 4 * g; q += LD_NT) stage[q >> 2][q & 3] = a.ends[(row * a.G) * 4 + q];
            __syncthreads();
            if (tid == 0) {
                double s[4] = {0.0, 0.0, 0.0, 0.0};
                for (int q = 0; q < g; ++q) {
                    double n[4];
                    ld_matvec(t.MS, s, n);
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i] = n[i] + stage[q][i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) start[i] = s[i];
            }
        }
        __syncthreads();
        if (g > 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = start[i];
        }
    }
    float scale2 = 0.f;
    const float* __restrict__ cov = nullptr;
    if (BWD) {
        scale2 = 2.f * a.gL[row / a.chs];
        cov = a.cov + row * a.nsub;
    }
    double* __restrict__ part = (EPI == LD_SUMS || EPI == LD_SUMS_STORE) ? a.partial + row * (long)a.nq * LD_BINS : nullptr;
    float* __restrict__ wimg = img[w];

    for (int tile = 0; tile < ntiles; ++tile) {
        const int par = tile & 1;
        const int m0 = mseg + tile * LD_TILE + tid * LD_L;           // logical position of the chunk's first sample
        const int nlo = BWD ? N - m0 - LD_L : m0;                    // lowest sample index of the chunk (may leave the row when ragged)
        const bool full = m0 + LD_L <= N;
        const int wm0 = m0 - lane * LD_L;                            // the wave's first logical position
        const bool wfull = wm0 + 64 * LD_L <= N;                     // the wave's 2048 samples lie inside the row (wave-uniform)
        const int wlo = BWD ? N - wm0 - 64 * LD_L : wm0;             // their lowest sample index
        const int cidx = BWD ? 63 - lane : lane;                     // this lane's chunk in memory order
        float X[LD_L];                                               // in memory order
        if (wfull) {                                                 // coalesced 16-byte loads, transposed through the wave's LDS image
            const f4u* __restrict__ p = reinterpret_cast<const f4u*>(in + wlo);
            f4u q[LD_L / 4];
#pragma unroll
            for (int v = 0; v < LD_L / 4; ++v) q[v] = __builtin_nontemporal_load(p + v * 64 + lane);
            wave_lds_sync();
#pragma unroll
            for (int v = 0; v < LD_L / 4; ++v)
                *reinterpret_cast<f4*>(wimg + (v * 8 + (lane >> 3)) * LD_PITCH + 4 * (lane & 7)) = f4{q[v].x, q[v].y, q[v].z, q[v].w};
            wave_lds_sync();
#pragma unroll
            for (int v = 0; v < LD_L / 4; ++v) {
                const f4 r = *reinterpret_cast<const f4*>(wimg + cidx * LD_PITCH + 4 * v);
                X[4 * v] = r.x; X[4 * v + 1] = r.y; X[4 * v + 2] = r.z; X[4 * v + 3] = r.w;
            }
        } else if (full) {
            const f4u* __restrict__ p = reinterpret_cast<const f4u*>(in + nlo);
#pragma unroll
            for (int v = 0; v < LD_L / 4; ++v) {
                const f4u q = __builtin_nontemporal_load(p + v);
                X[4 * v] = q.x; X[4 * v + 1] = q.y; X[4 * v + 2] = q.z; X[4 * v + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < LD_L; ++k) {
                const int n = nlo + k;
                X[k] = (n >= 0 && n < N && m0 < N) ? in[n] : 0.f;
            }
        }
        // sub-blocks of the chunk: samples below index nlo + kb belong to sub-block sa, the rest to sa + 1
        int sa = 0, kb = LD_L;
        if (EPI != LD_STATE || BWD) {
            const int nl = nlo > 0 ? nlo : 0;
            sa = (int)((unsigned)nl / (unsigned)H);
            kb = (sa + 1) * H - nlo;
        }
        if (BWD) {
            const float wa = scale2 * (sa < a.nsub ? cov[sa] : 0.f);            // (the ignored tail too is multiplied: a NaN there, or a NaN
            const float wb = scale2 * (sa + 1 < a.nsub ? cov[sa + 1] : 0.f);    // upstream gradient, reaches the whole row as in u = 2 y w gL)
#pragma unroll
            for (int k = 0; k < LD_L; ++k) X[k] *= (k < kb ? wa : wb);
        }
        double e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < LD_L; ++k) {
            const int i = BWD ? LD_L - 1 - k : k;
            X[i] = (float)ld_step(t.c, e, (double)X[i]);
        }
        // inclusive scan of the end states over the wave: E[l] = sum_{j <= l} M^(32 (l - j)) e[j]
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double v[4], o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = __shfl_up(e[i], 1 << k, 64);
            ld_matvec(Pl[k], v, o);
            if (lane >= (1 << k)) {
#pragma unroll
                for (int i = 0; i < 4; ++i) e[i] += o[i];
            }
        }
        double prev[4];
        if (EPI != LD_STATE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double v = __shfl_up(e[i], 1, 64);
                prev[i] = lane ? v : 0.0;
            }
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < 4; ++i) tot[par][w][i] = e[i];
        }
        __syncthreads();
        // the state at the start of this wave, and of the next tile
        double mine[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int v = 0; v < LD_NW; ++v) {
            if (v == w) {
#pragma unroll
                for (int i = 0; i < 4; ++i) mine[i] = c[i];
            }
            double n[4];
            ld_matvec(Pl[6], c, n);
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = n[i] + tot[par][v][i];
        }
        if (EPI == LD_STATE) continue;
        float sf[4];
        {
            double s[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                s[i] = fma(Q[4 * i + 3][lane], mine[3], fma(Q[4 * i + 2][lane], mine[2], fma(Q[4 * i + 1][lane], mine[1], fma(Q[4 * i][lane], mine[0], prev[i]))));
#pragma unroll
            for (int i = 0; i < 4; ++i) sf[i] = (float)s[i];
        }
#pragma unroll
        for (int k = 0; k < LD_L; ++k) {
            const int i = BWD ? LD_L - 1 - k : k;
            const f4 r = *reinterpret_cast<const f4*>(Rl[k]);
            X[i] = fmaf(r.w, sf[3], fmaf(r.z, sf[2], fmaf(r.y, sf[1], fmaf(r.x, sf[0], X[i]))));
        }
        if (EPI == LD_SUMS_STORE || EPI == LD_STORE) {
            if (wfull) {
                wave_lds_sync();
#pragma unroll
                for (int v = 0; v < LD_L / 4; ++v)
                    *reinterpret_cast<f4*>(wimg + cidx * LD_PITCH + 4 * v) = f4{X[4 * v], X[4 * v + 1], X[4 * v + 2], X[4 * v + 3]};
                wave_lds_sync();
                f4u* __restrict__ p = reinterpret_cast<f4u*>(out + wlo);
#pragma unroll
                for (int v = 0; v < LD_L / 4; ++v) {
                    const f4 r = *reinterpret_cast<const f4*>(wimg + (v * 8 + (lane >> 3)) * LD_PITCH + 4 * (lane & 7));
                    __builtin_nontemporal_store(f4u{r.x, r.y, r.z, r.w}, p + v * 64 + lane);
                }
            } else if (full) {
                f4u* __restrict__ p = reinterpret_cast<f4u*>(out + nlo);
#pragma unroll
                for (int v = 0; v < LD_L / 4; ++v) __builtin_nontemporal_store(f4u{X[4 * v], X[4 * v + 1], X[4 * v + 2], X[4 * v + 3]}, p + v);
            } else {
#pragma unroll
                for (int k = 0; k < LD_L; ++k) {
                    const int n = nlo + k;
                    if (n >= 0 && n < N && m0 < N) out[n] = X[k];
                }
            }
        }
        if (EPI == LD_SUMS || EPI == LD_SUMS_STORE) {
            const int nvalid = N - m0 < LD_L ? (N - m0 > 0 ? N - m0 : 0) : LD_L;     // the filter rings on behind the row's end
            float qa = 0.f, qb = 0.f;
#pragma unroll
            for (int k = 0; k < LD_L; ++k) {
                const float sq = X[k] * X[k];
                qa += (k < kb && k < nvalid) ? sq : 0.f;
                qb += (k >= kb && k < nvalid) ? sq : 0.f;
            }
            double da = (double)qa, db = (double)qb;
            if (qa == INFINITY || qb == INFINITY) {          // a square (|y| > 1.8e19) or their sum left float32: these 32 again, in fp64
                da = db = 0.0;
#pragma unroll
                for (int k = 0; k < LD_L; ++k) {
                    const double sq = (double)X[k] * (double)X[k];
                    da += (k < kb && k < nvalid) ? sq : 0.0;
                    db += (k >= kb && k < nvalid) ? sq : 0.0;
                }
            }
            // the wave's sums of the (at most four) sub-blocks its samples fall in, bin 0 = the sub-block of its first sample; the gate
            // launch adds the waves of a row up in sequence
            const int sw = __builtin_amdgcn_readfirstlane(sa);
#pragma unroll
            for (int k = 0; k < LD_BINS; ++k) {
                double v = (sa - sw == k ? da : 0.0) + (sa + 1 - sw == k ? db : 0.0);
                v = wave_sum(v);
                if (lane == 0 && wm0 < N) part[(long)(wm0 / (64 * LD_L)) * LD_BINS + k] = v;
            }
        }
    }
    if (EPI == LD_STATE) {
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a.ends[(row * a.G + g) * 4 + i] = c[i];
        }
    }
}

// ---- gates ----------------------------------------------------------------------------------------------------------------------------
constexpr int LG_NT = 256;

struct LgArgs {
    const double* partial;      // (items * chs, nq, 4)
    double* sub;                // (items * chs, nsub): the sub-block sums, segments combined
    float* L;                   // (items)
    float* cov;                 // (items * chs, nsub) or NULL
    int H, nsub, chs, nq, nb;
    double w[LD_MAX_CH];
};

__device__ __forceinline__ double lg_block_sum(double v, double* red) {      // fixed order: wave tree, then the waves in sequence; all threads get it
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    double s = red[0];
    for (int k = 1; k < LG_NT / 64; ++k) s += red[k];
    return s;
}
__device__ __forceinline__ double lg_power(const LgArgs& a, const double* __restrict__ sub, int j) {     // p[j] = sum_c G_c z[c, j]
    double p = 0.0;
    for (int ch = 0; ch < a.chs; ++ch) {
        const double* s = sub + (long)ch * a.nsub + j;
        p += a.w[ch] * ((((s[0] + s[1]) + s[2]) + s[3]) / (4.0 * a.H));
    }
    return p;
}
__device__ __forceinline__ double lg_lufs(double p) { return -0.691 + 10.0 * log10(p); }

__global__ void __launch_bounds__(LG_NT) ld_gate_kernel(const LgArgs a) {
    __shared__ double red[LG_NT / 64];
    const long item = blockIdx.x;
    const int tid = threadIdx.x;
    double* __restrict__ sub = a.sub + item * a.chs * (long)a.nsub;
    for (int q = tid; q < a.chs * a.nsub; q += LG_NT) {
        const int ch = q / a.nsub, s = q - ch * a.nsub;
        const long row = item * a.chs + ch;
        const int W = 64 * LD_L;                                   // sub-block s holds samples of the waves qlo .. qhi of the row
        const int qlo = (int)(((long)s * a.H) / W), qhi = (int)((((long)s + 1) * a.H - 1) / W);
        double acc = 0.0;
        for (int v = qlo; v <= qhi; ++v) acc += a.partial[(row * a.nq + v) * LD_BINS + (s - (int)(((long)v * W) / a.H))];
        sub[q] = acc;
    }
    __syncthreads();
    double sumA = 0.0, cntA = 0.0;
    for (int j = tid; j < a.nb; j += LG_NT) {
        const double p = lg_power(a, sub, j);
        if (lg_lufs(p) > -70.0) { sumA += p; cntA += 1.0; }
    }
    sumA = lg_block_sum(sumA, red);
    cntA = lg_block_sum(cntA, red);
    double L = -INFINITY, dz = 0.0, gamma = INFINITY;
    if (cntA > 0.0) {
        gamma = lg_lufs(sumA / cntA) - 10.0;
        double sumJ = 0.0, cntJ = 0.0;
        for (int j = tid; j < a.nb; j += LG_NT) {
            const double p = lg_power(a, sub, j), l = lg_lufs(p);
            if (l > -70.0 && l > gamma) { sumJ += p; cntJ += 1.0; }
        }
        sumJ = lg_block_sum(sumJ, red);
        cntJ = lg_block_sum(cntJ, red);
        if (cntJ > 0.0) {
            L = lg_lufs(sumJ / cntJ);
            dz = 4.342944819032518 / sumJ / (4.0 * a.H);          // (10 / ln 10) / (|J| P) / T
        }
    }
    if (tid == 0) a.L[item] = (float)L;
    if (a.cov) {
        for (int q = tid; q < a.chs * a.nsub; q += LG_NT) {
            const int ch = q / a.nsub, s = q - ch * a.nsub;
            int cnt = 0;
            if (dz != 0.0)
                for (int j = s - 3 > 0 ? s - 3 : 0; j <= s && j < a.nb; ++j) {
                    const double l = lg_lufs(lg_power(a, sub, j));
                    cnt += (l > -70.0 && l > gamma) ? 1 : 0;
                }
            a.cov[(item * a.chs + ch) * (long)a.nsub + s] = dz != 0.0 ? (float)(dz * a.w[ch] * cnt) : -0.f;      // -0.f: LD_EMPTY_GATE
        }
    }
}

// ---- peak normalisation ---------------------------------------------------------------------------------------------------------------
constexpr int PK_NT = 256;
constexpr long PK_MIN_SEG = 4096;

struct PkSpan {
    long off;
    int s0, len, nvec;
};
__device__ __forceinline__ PkSpan pk_span(long N, long S, long G) {
    PkSpan s;
    const long r = (long)blockIdx.x / G, g = (long)blockIdx.x - r * G;
    s.s0 = (int)(g * S);
    s.off = r * N + s.s0;
    s.len = (int)(N - s.s0 < S ? N - s.s0 : S);
    s.nvec = s.len >> 2;
    return s;
}
// (max, lowest index attaining it): the order of combination does not matter, the result is exact
__device__ __forceinline__ void pk_take(float& m, int& k, float v, int i) {
    if (v > m || (v == m && i < k)) { m = v; k = i; }
}
// A NaN sample makes the peak NaN (as torch.max does; fmaxf would drop it). Through the reduction it travels as +inf at a NEGATIVE index
// (the sample's index with PK_NAN set: in-row indices stay below 2^30), which wins every tie with a true inf; pk_peak turns it back.
constexpr int PK_NAN = (int)0x80000000;
__device__ __forceinline__ void pk_see(float& m, int& k, float v, int i) {
    const bool nan = v != v;
    pk_take(m, k, nan ? INFINITY : fabsf(v), nan ? (i | PK_NAN) : i);
}
__device__ __forceinline__ double pk_peak(float m, int& k) {
    if (k >= 0) return (double)m;
    k &= ~PK_NAN;
    return (double)NAN;
}

// MODE 0: partials[(r G + g) 2 + {0, 1}] = (max |x|, its lowest index) as doubles;  MODE 1: partials[r G + g] = sum g x (fp64, fixed order)
template <int MODE>
__global__ void __launch_bounds__(PK_NT) pk_reduce_kernel(const float* __restrict__ x, const float* __restrict__ gy, double* __restrict__ partials,
                                                          long N, long S, long G) {
    __shared__ double red[PK_NT / 64][2];
    const PkSpan s = pk_span(N, S, G);
    const int tid = threadIdx.x;
    const f4u* __restrict__ xv = reinterpret_cast<const f4u*>(x + s.off);
    const f4u* __restrict__ gv = reinterpret_cast<const f4u*>(MODE == 1 ? gy + s.off : x);
    float m = -1.f;
    int k = 0x7fffffff;
    double acc = 0.0;
    for (int v = tid; v < s.nvec; v += PK_NT) {
        const f4u q = __builtin_nontemporal_load(xv + v);
        if (MODE == 0) {
            pk_see(m, k, q.x, s.s0 + 4 * v);
            pk_see(m, k, q.y, s.s0 + 4 * v + 1);
            pk_see(m, k, q.z, s.s0 + 4 * v + 2);
            pk_see(m, k, q.w, s.s0 + 4 * v + 3);
        } else {
            const f4u h = __builtin_nontemporal_load(gv + v);
            acc += (double)fmaf(q.w, h.w, fmaf(q.z, h.z, fmaf(q.y, h.y, q.x * h.x)));
        }
    }
    const int i = 4 * s.nvec + tid;
    if (tid < 4 && i < s.len) {
        if (MODE == 0) pk_see(m, k, x[s.off + i], s.s0 + i);
        else acc += (double)(x[s.off + i] * gy[s.off + i]);
    }
    if (MODE == 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) pk_take(m, k, __shfl_down(m, d, 64), __shfl_down(k, d, 64));
        if (lane_id() == 0) { red[wave_id()][0] = (double)m; red[wave_id()][1] = (double)k; }
    } else {
        acc = wave_sum(acc);
        if (lane_id() == 0) red[wave_id()][0] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        if (MODE == 0) {
            for (int wv = 0; wv < PK_NT / 64; ++wv) pk_take(m, k, (float)red[wv][0], (int)red[wv][1]);
            partials[(long)blockIdx.x * 2] = (double)m;
            partials[(long)blockIdx.x * 2 + 1] = (double)k;
        } else {
            double tot = red[0][0];
            for (int wv = 1; wv < PK_NT / 64; ++wv) tot += red[wv][0];
            partials[blockIdx.x] = tot;
        }
    }
}

// MODE 0: y = x * scale / max(p, eps), peak[r] = (p, k) saved for the backward pass; p is NaN for a row that holds a NaN (y is NaN throughout)
// MODE 1: gx = scale (g / p - [n == k] sign(x[k]) D / p^2) for p > eps, scale g / eps for p <= eps, NaN throughout for a NaN p (src = g)
template <int MODE>
__global__ void __launch_bounds__(PK_NT) pk_apply_kernel(const float* __restrict__ src, const float* __restrict__ x, const double* __restrict__ partials,
                                                         double* __restrict__ peak, float* __restrict__ dst, long N, long S, long G, double scale,
                                                         double eps) {
    __shared__ float mul_s, fix_s;
    __shared__ int k_s;
    const PkSpan s = pk_span(N, S, G);
    const int tid = threadIdx.x;
    const long r = (long)blockIdx.x / G;
    if (tid == 0) {
        if (MODE == 0) {
            float m = -1.f;
            int k = 0x7fffffff;
            for (long g = 0; g < G; ++g) pk_take(m, k, (float)partials[(r * G + g) * 2], (int)partials[(r * G + g) * 2 + 1]);
            const double p = pk_peak(m, k);                  // NaN for a row that holds one, k then the index of its first NaN
            if (s.s0 == 0) { peak[2 * r] = p; peak[2 * r + 1] = (double)k; }
            mul_s = (float)(scale / (p <= eps ? eps : p));   // (not p > eps ? p : eps, which reads a NaN peak as silence)
            k_s = -1;
            fix_s = 0.f;
        } else {
            const double p = peak[2 * r];
            const int k = (int)peak[2 * r + 1];
            if (!(p <= eps)) {                               // a NaN peak comes this way too: mul_s and fix_s are NaN, and so is the row
                double D = 0.0;
                for (long g = 0; g < G; ++g) D += partials[r * G + g];
                const float xk = x[r * N + k];
                mul_s = (float)(scale / p);
                fix_s = (float)(-(xk < 0.f ? -1.0 : 1.0) * scale * D / (p * p));
                k_s = k;
            } else {
                mul_s = (float)(scale / eps);
                fix_s = 0.f;
                k_s = -1;
            }
        }
    }
    __syncthreads();
    const float mul = mul_s, fix = fix_s;
    const int kk = k_s - s.s0;                              // the index of the maximum relative to this segment
    const f4u* __restrict__ sv = reinterpret_cast<const f4u*>(src + s.off);
    f4u* __restrict__ dv = reinterpret_cast<f4u*>(dst + s.off);
    for (int v = tid; v < s.nvec; v += PK_NT) {
        f4u q = __builtin_nontemporal_load(sv + v);
        q.x *= mul; q.y *= mul; q.z *= mul; q.w *= mul;
        if (MODE == 1 && k_s >= 0 && (kk >> 2) == v && kk >= 0) {
            if ((kk & 3) == 0) q.x += fix;
            if ((kk & 3) == 1) q.y += fix;
            if ((kk & 3) == 2) q.z += fix;
            if ((kk & 3) == 3) q.w += fix;
        }
        __builtin_nontemporal_store(q, dv + v);
    }
    const int i = 4 * s.nvec + tid;
    if (tid < 4 && i < s.len) {
        float q = src[s.off + i] * mul;
        if (MODE == 1 && k_s >= 0 && kk == i) q += fix;
        dst[s.off + i] = q;
    }
}

// ---- host: the filter's tables and the plans --------------------------------------------------------------------------------------------
void kw_design(double fs, double (&c)[2][5]) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Qf = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Qf + K * K;
        c[0][0] = (Vh + Vb * K / Qf + K * K) / a0;
        c[0][1] = 2.0 * (K * K - Vh) / a0;
        c[0][2] = (Vh - Vb * K / Qf + K * K) / a0;
        c[0][3] = 2.0 * (K * K - 1.0) / a0;
        c[0][4] = (1.0 - K / Qf + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Qf = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), d = 1.0 + K / Qf + K * K;
        c[1][0] = 1.0; c[1][1] = -2.0; c[1][2] = 1.0;
        c[1][3] = 2.0 * (K * K - 1.0) / d;
        c[1][4] = (1.0 - K / Qf + K * K) / d;
    }
}
double kw_step(const double (&c)[2][5], double (&s)[4], double x) {
    const double ya = c[0][0] * x + s[0];
    s[0] = c[0][1] * x - c[0][3] * ya + s[1];
    s[1] = c[0][2] * x - c[0][4] * ya;
    const double yb = c[1][0] * ya + s[2];
    s[2] = c[1][1] * ya - c[1][3] * yb + s[3];
    s[3] = c[1][2] * ya - c[1][4] * yb;
    return yb;
}
void mat_mul(const double* A, const double* B, double* C) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += A[4 * i + k] * B[4 * k + j];
            r[4 * i + j] = acc;
        }
    for (int i = 0; i < 16; ++i) C[i] = r[i];
}
void mat_pow(const double* M, long n, double* out) {
    double base[16], acc[16];
    for (int i = 0; i < 16; ++i) { base[i] = M[i]; acc[i] = (i % 5 == 0) ? 1.0 : 0.0; }
    for (; n > 0; n >>= 1) {
        if (n & 1) mat_mul(base, acc, acc);
        mat_mul(base, base, base);
    }
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
}
void kw_tables(double fs, long S, LdTab* t) {
    kw_design(fs, t->c);
    double M[16];
    for (int j = 0; j < 4; ++j) {                  // column j: one step from the unit state e_j with no input
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[j] = 1.0;
        kw_step(t->c, s, 0.0);
        for (int i = 0; i < 4; ++i) M[4 * i + j] = s[i];
    }
    for (int j = 0; j < 4; ++j) {                  // the output's response to the unit states
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[j] = 1.0;
        for (int k = 0; k < LD_L; ++k) t->R[k][j] = (float)kw_step(t->c, s, 0.0);
    }
    mat_pow(M, LD_L, t->P[0]);
    for (int k = 1; k < LD_NP; ++k) mat_mul(t->P[k - 1], t->P[k - 1], t->P[k]);
    mat_pow(M, S, t->MS);
}

struct LdPlan {
    int H, nb, nsub, S, G, nq;
};
bool ld_plan_segments(long rows, long N, int* S, int* G) {
    if (rows < 1 || N < 1 || N > LD_MAX_N || rows > (1L << 40) / N) return false;
    long s = N, g = 1;
    if (rows < LD_FILL / 2 && N >= 2 * LD_TILE) {        // fewer rows than fill the chip, and long enough to cut
        const long want = (LD_FILL + rows - 1) / rows;
        s = (N + want - 1) / want;
        s = (s + LD_TILE - 1) / LD_TILE * LD_TILE;
        g = (N + s - 1) / s;
        while (g > LD_MAX_SEG) {
            s += LD_TILE;
            g = (N + s - 1) / s;
        }
    }
    if (rows * g > 0x7fffffffL) return false;
    *S = (int)s;
    *G = (int)g;
    return true;
}
bool ld_plan(long items, int chs, long N, double fs, LdPlan* p) {
    if (items < 1 || chs < 1 || chs > LD_MAX_CH || !(fs >= 8000.0) || !(fs <= 384000.0)) return false;
    p->H = (int)floor(0.1 * fs + 0.5);
    if (N < 4L * p->H) return false;
    if (!ld_plan_segments(items * chs, N, &p->S, &p->G)) return false;
    p->nb = (int)((N - 4L * p->H) / p->H) + 1;
    p->nsub = p->nb + 3;
    p->nq = (int)((N + 64 * LD_L - 1) / (64 * LD_L));
    return true;
}
// doubles of scratch: per-wave sub-block sums, combined sub-block sums, segment end states
long ld_scratch(long items, int chs, const LdPlan& p) {
    const long rows = items * chs;
    return rows * p.nq * LD_BINS + rows * p.nsub + rows * p.G * 4;
}

bool pk_plan(long rows, long N, long* S, long* G) {
    if (rows < 1 || N < 1 || N > LD_MAX_N || rows > (1L << 40) / N) return false;
    const long want = (LD_FILL + rows - 1) / rows;
    long s = (N + want - 1) / want;
    if (s < PK_MIN_SEG) s = PK_MIN_SEG;
    s = (s + 1023) / 1024 * 1024;
    *S = s;
    *G = (N + s - 1) / s;
    return rows * *G <= 0x7fffffffL;
}

int ld_check() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DASP_OK : (int)e;
}

const double LD_CH_WEIGHTS[LD_MAX_CH] = {1.0, 1.0, 1.0, 1.41, 1.41};

}  // namespace

extern "C" {

int dasp_loudness_kweighting(double sample_rate, double* sos12) {
    if (!sos12 || !(sample_rate >= 8000.0) || !(sample_rate <= 384000.0)) return DASP_ERR_ARG;
    double c[2][5];
    kw_design(sample_rate, c);
    for (int s = 0; s < 2; ++s) {
        sos12[6 * s + 0] = c[s][0]; sos12[6 * s + 1] = c[s][1]; sos12[6 * s + 2] = c[s][2];
        sos12[6 * s + 3] = 1.0; sos12[6 * s + 4] = c[s][3]; sos12[6 * s + 5] = c[s][4];
    }
    return DASP_OK;
}

long dasp_loudness_blocks(long N, double sample_rate) {
    LdPlan p;
    return ld_plan(1, 1, N, sample_rate, &p) ? p.nb : -1;
}

long dasp_loudness_segments(long rows, long N) {
    int S, G;
    return ld_plan_segments(rows, N, &S, &G) ? G : -1;
}

long dasp_loudness_scratch_doubles(long items, int chs, long N, double sample_rate) {
    LdPlan p;
    return ld_plan(items, chs, N, sample_rate, &p) ? ld_scratch(items, chs, p) : -1;
}

int dasp_loudness_forward(const float* x, double* scratch, float* L, float* ysave, float* cov, long items, int chs, long N, double sample_rate,
                          void* stream) {
    if (!x || !scratch || !L || items < 1 || N < 1 || (ysave == nullptr) != (cov == nullptr)) return DASP_ERR_ARG;
    LdPlan p;
    if (!ld_plan(items, chs, N, sample_rate, &p)) return DASP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long rows = items * chs;
    LdTab t;
    kw_tables(sample_rate, p.S, &t);
    LdArgs a = {};
    a.in = x; a.out = ysave;
    a.partial = scratch;
    double* sub = scratch + rows * p.nq * LD_BINS;
    a.ends = sub + rows * p.nsub;
    a.N = (int)N; a.S = p.S; a.G = p.G; a.H = p.H; a.nsub = p.nsub; a.chs = chs; a.nq = p.nq;
    if (p.G > 1)
        hipLaunchKernelGGL((ld_filter_kernel<false, LD_STATE>), dim3((unsigned)(rows * (p.G - 1))), dim3(LD_NT), 0, st, a, t);
    if (ysave)
        hipLaunchKernelGGL((ld_filter_kernel<false, LD_SUMS_STORE>), dim3((unsigned)(rows * p.G)), dim3(LD_NT), 0, st, a, t);
    else
        hipLaunchKernelGGL((ld_filter_kernel<false, LD_SUMS>), dim3((unsigned)(rows * p.G)), dim3(LD_NT), 0, st, a, t);
    LgArgs q = {};
    q.partial = scratch; q.sub = sub; q.L = L; q.cov = cov;
    q.H = p.H; q.nsub = p.nsub; q.chs = chs; q.nq = p.nq; q.nb = p.nb;
    for (int c = 0; c < LD_MAX_CH; ++c) q.w[c] = LD_CH_WEIGHTS[c];
    hipLaunchKernelGGL(ld_gate_kernel, dim3((unsigned)items), dim3(LG_NT), 0, st, q);
    return ld_check();
}

int dasp_loudness_backward(const float* ysave, const float* cov, const float* gL, double* scratch, float* gx, long items, int chs, long N,
                           double sample_rate, void* stream) {
    if (!ysave || !cov || !gL || !scratch || !gx || items < 1 || N < 1) return DASP_ERR_ARG;
    LdPlan p;
    if (!ld_plan(items, chs, N, sample_rate, &p)) return DASP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long rows = items * chs;
    LdTab t;
    kw_tables(sample_rate, p.S, &t);
    LdArgs a = {};
    a.in = ysave; a.out = gx; a.cov = cov; a.gL = gL;
    a.ends = scratch + rows * p.nq * LD_BINS + rows * p.nsub;
    a.N = (int)N; a.S = p.S; a.G = p.G; a.H = p.H; a.nsub = p.nsub; a.chs = chs; a.nq = p.nq;
    if (p.G > 1)
        hipLaunchKernelGGL((ld_filter_kernel<true, LD_STATE>), dim3((unsigned)(rows * (p.G - 1))), dim3(LD_NT), 0, st, a, t);
    hipLaunchKernelGGL((ld_filter_kernel<true, LD_STORE>), dim3((unsigned)(rows * p.G)), dim3(LD_NT), 0, st, a, t);
    return ld_check();
}

long dasp_peaknorm_scratch_doubles(long rows, long N) {
    long S, G;
    return pk_plan(rows, N, &S, &G) ? 2 * rows * G : -1;
}

int dasp_peaknorm_forward(const float* x, double* scratch, double* peak, float* y, long rows, long N, double peak_db, double eps, void* stream) {
    if (!x || !scratch || !peak || !y || rows < 1 || N < 1 || !isfinite(peak_db) || !(eps >= 0.0)) return DASP_ERR_ARG;
    long S, G;
    if (!pk_plan(rows, N, &S, &G)) return DASP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(rows * G));
    hipLaunchKernelGGL(pk_reduce_kernel<0>, grid, dim3(PK_NT), 0, st, x, (const float*)nullptr, scratch, N, S, G);
    hipLaunchKernelGGL(pk_apply_kernel<0>, grid, dim3(PK_NT), 0, st, x, x, (const double*)scratch, peak, y, N, S, G, pow(10.0, peak_db / 20.0), eps);
    return ld_check();
}

int dasp_peaknorm_backward(const float* x, const float* gy, const double* peak, double* scratch, float* gx, long rows, long N, double peak_db,
                           double eps, void* stream) {
    if (!x || !gy || !peak || !scratch || !gx || rows < 1 || N < 1 || !isfinite(peak_db) || !(eps >= 0.0)) return DASP_ERR_ARG;
    long S, G;
    if (!pk_plan(rows, N, &S, &G)) return DASP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(rows * G));
    hipLaunchKernelGGL(pk_reduce_kernel<1>, grid, dim3(PK_NT), 0, st, x, gy, scratch, N, S, G);
    hipLaunchKernelGGL(pk_apply_kernel<1>, grid, dim3(PK_NT), 0, st, gy, x, (const double*)scratch, (double*)peak, gx, N, S, G,
                       pow(10.0, peak_db / 20.0), eps);
    return ld_check();
}

}  // extern "C"
