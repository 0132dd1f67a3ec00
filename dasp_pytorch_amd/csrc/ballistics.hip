// block_level and ballistics: the detector and the attack / release smoother of the control-rate layer. audio -> curve and curve -> curve.
// Frame conventions of envelope.hip: h = hop, F = ceil(N / h) + 1 frame points, frame point j at sample j h.
//
// BLOCK_LEVEL. With p[m] = max_c |x[b,c,m]| (peak; the lowest channel wins a tie, the first NaN channel makes p NaN) or mean_c x[b,c,m]^2
// (power), p = 0 from sample N on:
//   L[b,0] = p[0];   L[b,j] = max_{i=1..h} p[(j-1) h + i]  (peak)  |  (1 / h) sum_{i=1..h} p[(j-1) h + i]  (power),   j = 1 .. F-1
// FORWARD (blocklevel_forward_kernel): the tile walk of envelope_block_kernel - one workgroup per (item, tile of 4096 samples from sample
//   4096 k + 1 on), all channels, whole hops per tile. The per-sample level goes through LDS (a lane per consecutive sample on the global
//   side, 16 consecutive samples per thread on the other). Peak carries the winner: the signed sample and its channel are staged, a
//   candidate replaces the current winner when (a > cur) | (isnan(a) & !isnan(cur)), candidates are met in time order - a thread's run of
//   samples, then the threads of a block on DPP row shifts and row broadcasts, then two waves through LDS (hop 2048) - so the earliest
//   sample that holds the maximum wins, on its lowest winning channel, and the first NaN sample of a block wins it. The winner is saved
//   as one word per frame, (i - 1) | sign << 11 | channel << 13 for the sample (j-1) h + i, sign 0 zero, 1 positive, 2 negative, 3 NaN:
//   the backward pass needs nothing else. Power adds the 16 samples of a thread as two runs of 8, each in time order, and the threads of
//   a block as a balanced tree (the same DPP steps), then scales by 1 / h: float32, one fixed order.
// BACKWARD: peak is a write-only pass (blocklevel_peak_backward_kernel): every thread decides from its hop's saved winner whether its
//   sample is the winner, gx = sign(x_winner) gL_j there and a written zero everywhere else. Power reads x:
//   gx = (2 / (chs h) gL_j) x, and (2 / chs gL_0) x for sample 0.
//
// BALLISTICS. For item b over the F values of a curve P, E_{-1} = 0:
//   t_a = clamp(attack_ms, 0.1, 10000);   c_a = -expm1(-ln 9 hop / (sr t_a / 1000));   c_r likewise from release_ms
//   up_j = P_j > E_{j-1};   c_j = up_j ? c_a : c_r;   E_j = E_{j-1} + c_j (P_j - E_{j-1})
// A composition of these max-of-affine maps has no fixed-size form, so there is no scan: one workgroup of one wave per item, the curve
// staged through LDS in chunks of 1024 frames with coalesced loads (the next chunk's loads are in flight while this one is walked), lane
// 0 walks the recurrence in float64 without contraction (the products and sums round as written), E (rounded once to float32) and the
// mask go back out through LDS with coalesced stores. BACKWARD walks the chunks in reverse, the same way:
//   Lambda_j = gE_j + (1 - c_{j+1}) Lambda_{j+1};   gP_j = c_j Lambda_j
//   g_attack = (dc_a/dt_a) sum_{j: up_j} Lambda_j (P_j - E_{j-1}),   g_release over the other frames,   dc/dt = -(1-c) ln 9 hop 1000 / (sr t^2)
// with the saved mask and the saved float32 E, the recurrence and both sums in float64 in the order j = F-1 .. 0.
//
// No atomics anywhere: every result is bit-identical run to run and for an item alone or in a batch.
#include "row_helpers.hpp"

namespace dasp {

constexpr int BL_THREADS = 256;
constexpr int BL_SPT = 16;                            // consecutive samples per thread
constexpr int BL_TILE = BL_THREADS * BL_SPT;          // 4096: a multiple of every hop, dasp_envelope_tile()
constexpr int BL_RUN = 8;                             // the smallest hop
constexpr int BL_NW = BL_THREADS / 64;
constexpr int BL_STAGE = BL_TILE + BL_TILE / BL_SPT;
constexpr int BL_MAX_CH = 1 << 18;                    // the winner's word holds the channel in 18 bits

constexpr int BAL_CHUNK = 1024;                       // frames per staged chunk
constexpr int BAL_PER = BAL_CHUNK / 64;               // per lane

__host__ __device__ inline bool bl_hop_ok(int hop) { return hop >= 8 && hop <= 2048 && !(hop & (hop - 1)); }
__host__ __device__ inline long bl_frames(long N, int hop) { return (N + hop - 1) / hop + 1; }

// ---- block_level ------------------------------------------------------------------------------------------------------------------------
// a winner: the signed sample (its magnitude is the level) and where it lies, block position | channel << 11
struct BlWin { float v; int at; };

__device__ __forceinline__ bool bl_replaces(float a, float cur) { return (a > cur) | ((a != a) & (cur == cur)); }
// `late` follows `early` in time
__device__ __forceinline__ BlWin bl_meet(const BlWin& early, const BlWin& late) { return bl_replaces(fabsf(late.v), fabsf(early.v)) ? late : early; }
__device__ __forceinline__ int bl_word(const BlWin& w) {
    const int s = w.v != w.v ? 3 : (w.v > 0.f ? 1 : (w.v < 0.f ? 2 : 0));
    return (w.at & 2047) | s << 11 | (w.at >> 11) << 13;
}

// (a lane without a source gets zeros; the last lane of a group, the one that is read, always has one)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ BlWin bl_dpp(const BlWin& w) {
    BlWin o;
    o.v = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, w.v), CTRL, ROW_MASK, 0xf, false));
    o.at = __builtin_amdgcn_update_dpp(0, w.at, CTRL, ROW_MASK, 0xf, false);
    return o;
}
// the winner of groups of 2^k adjacent lanes, k = 0 .. 6, in the last lane of every group: the steps of env_group_sum
__device__ __forceinline__ BlWin bl_group_win(BlWin w, int k) {
    if (k >= 1) w = bl_meet(bl_dpp<0x111, 0xf>(w), w);       // row_shr:1
    if (k >= 2) w = bl_meet(bl_dpp<0x112, 0xf>(w), w);       // row_shr:2
    if (k >= 3) w = bl_meet(bl_dpp<0x114, 0xf>(w), w);       // row_shr:4
    if (k >= 4) w = bl_meet(bl_dpp<0x118, 0xf>(w), w);       // row_shr:8
    if (k >= 5) {                                            // row_bcast:15: rows 1 and 3 meet the row before them
        const BlWin o = bl_dpp<0x142, 0xa>(w);
        if ((threadIdx.x & 16) != 0) w = bl_meet(o, w);
    }
    if (k >= 6) {                                            // row_bcast:31: rows 2 and 3 meet rows 0 .. 1
        const BlWin o = bl_dpp<0x143, 0xc>(w);
        if ((threadIdx.x & 32) != 0) w = bl_meet(o, w);
    }
    return w;
}
__device__ __forceinline__ float bl_group_sum(float v, int k) {
    if (k >= 1) v += dpp_or_zero<0x111, 0xf>(v);
    if (k >= 2) v += dpp_or_zero<0x112, 0xf>(v);
    if (k >= 3) v += dpp_or_zero<0x114, 0xf>(v);
    if (k >= 4) v += dpp_or_zero<0x118, 0xf>(v);
    if (k >= 5) v += dpp_or_zero<0x142, 0xa>(v);
    if (k >= 6) v += dpp_or_zero<0x143, 0xc>(v);
    return v;
}

// the level of sample m alone and its winner (frame point 0)
template <bool PEAK> __device__ __forceinline__ float bl_sample(const float* __restrict__ xb, long N, int C, long m, float invC, BlWin& w) {
    const float v = xb[m];
    w.v = v; w.at = 0;
    float p = v * v;
    for (int c = 1; c < C; ++c) {
        const float o = xb[(size_t)c * N + m];
        if (PEAK) {
            if (bl_replaces(fabsf(o), fabsf(w.v))) { w.v = o; w.at = c << 11; }
        } else
            p = __builtin_fmaf(o, o, p);
    }
    return PEAK ? fabsf(w.v) : p * invC;
}

template <bool PEAK>
__global__ void __launch_bounds__(BL_THREADS)
blocklevel_forward_kernel(const float* __restrict__ x, float* __restrict__ L, int* __restrict__ win, long N, long F, int ntile, int C, int hop) {
    __shared__ float st[BL_STAGE];
    __shared__ int sc[PEAK ? BL_STAGE : 1];
    __shared__ float wv[BL_NW];
    __shared__ int wa[BL_NW];
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const float* xb = x + (size_t)b * C * N;
    const float invC = 1.f / (float)C;
    const long t0 = (long)tile * BL_TILE + 1;                             // block j covers samples (j - 1) h + 1 .. j h

    float pk[BL_SPT];
    int ch[BL_SPT];
    stage_load<BL_SPT, BL_THREADS>(pk, xb, t0, N, tid);
#pragma unroll
    for (int m = 0; m < BL_SPT; ++m) {
        ch[m] = 0;
        if (!PEAK) pk[m] = pk[m] * pk[m];
    }
    for (int c = 1; c < C; ++c) {
        float o[BL_SPT];
        stage_load<BL_SPT, BL_THREADS>(o, xb + (size_t)c * N, t0, N, tid);
#pragma unroll
        for (int m = 0; m < BL_SPT; ++m) {
            if (PEAK) {
                if (bl_replaces(fabsf(o[m]), fabsf(pk[m]))) { pk[m] = o[m]; ch[m] = c; }
            } else
                pk[m] = __builtin_fmaf(o[m], o[m], pk[m]);
        }
    }
    if (!PEAK) {
#pragma unroll
        for (int m = 0; m < BL_SPT; ++m) pk[m] *= invC;
    }
    stage_put<BL_SPT, BL_THREADS>(st, pk, tid);
    if (PEAK) {
#pragma unroll
        for (int m = 0; m < BL_SPT; ++m) sc[stage_word<BL_SPT>(tid + BL_THREADS * m)] = ch[m];
    }
    __syncthreads();

    float* Lb = L + (size_t)b * F;
    int* wb = PEAK && win ? win + (size_t)b * F : nullptr;
    const long j0 = (long)tile * (BL_TILE / hop) + 1;
    const int lane = tid & 63, wave = tid >> 6;
    const int lpb = hop / BL_SPT;                                          // threads per block (0: two blocks per thread)
    const float invh = 1.f / (float)hop;

    if (PEAK) {
        BlWin q[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int s = BL_SPT * tid + BL_RUN * r;
            q[r].v = st[stage_word<BL_SPT>(s)];
            q[r].at = (s & (hop - 1)) | sc[stage_word<BL_SPT>(s)] << 11;
#pragma unroll
            for (int i = 1; i < BL_RUN; ++i) {
                BlWin n;
                n.v = st[stage_word<BL_SPT>(s + i)];
                n.at = ((s + i) & (hop - 1)) | sc[stage_word<BL_SPT>(s + i)] << 11;
                q[r] = bl_meet(q[r], n);
            }
        }
        if (hop == BL_RUN) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const long j = j0 + 2 * tid + r;
                if (j < F) { Lb[j] = fabsf(q[r].v); if (wb) wb[j] = bl_word(q[r]); }
            }
        } else {
            BlWin w = bl_meet(q[0], q[1]);
            const int k = 31 - __builtin_clz(lpb < 64 ? lpb : 64);
            w = bl_group_win(w, k);
            if (lpb <= 64) {
                const long j = j0 + tid / lpb;
                if ((lane & (lpb - 1)) == lpb - 1 && j < F) { Lb[j] = fabsf(w.v); if (wb) wb[j] = bl_word(w); }
            } else {                                                       // hop 2048: two waves per block
                if (lane == 63) { wv[wave] = w.v; wa[wave] = w.at; }
                __syncthreads();
                if (tid < BL_NW / 2 && j0 + tid < F) {
                    BlWin e, l;
                    e.v = wv[2 * tid]; e.at = wa[2 * tid];
                    l.v = wv[2 * tid + 1]; l.at = wa[2 * tid + 1];
                    const BlWin r = bl_meet(e, l);
                    Lb[j0 + tid] = fabsf(r.v);
                    if (wb) wb[j0 + tid] = bl_word(r);
                }
            }
        }
    } else {
        float q[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int s = BL_SPT * tid + BL_RUN * r;
            float a = st[stage_word<BL_SPT>(s)];
#pragma unroll
            for (int i = 1; i < BL_RUN; ++i) a += st[stage_word<BL_SPT>(s + i)];
            q[r] = a;
        }
        if (hop == BL_RUN) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const long j = j0 + 2 * tid + r;
                if (j < F) Lb[j] = q[r] * invh;
            }
        } else {
            const int k = 31 - __builtin_clz(lpb < 64 ? lpb : 64);
            const float u = bl_group_sum(q[0] + q[1], k);
            if (lpb <= 64) {
                const long j = j0 + tid / lpb;
                if ((lane & (lpb - 1)) == lpb - 1 && j < F) Lb[j] = u * invh;
            } else {
                if (lane == 63) wv[wave] = u;
                __syncthreads();
                if (tid < BL_NW / 2 && j0 + tid < F) Lb[j0 + tid] = (wv[2 * tid] + wv[2 * tid + 1]) * invh;
            }
        }
    }
    if (tile == 0 && tid == 0) {                                          // frame point 0 is sample 0 alone
        BlWin w;
        Lb[0] = bl_sample<PEAK>(xb, N, C, 0, invC, w);
        if (wb) wb[0] = bl_word(w);
    }
}

// write-only: gx[b,c,m] = sign(x_winner) gL_j where (m, c) is the winner of frame j = ceil(m / h), a written zero elsewhere
__global__ void __launch_bounds__(BL_THREADS)
blocklevel_peak_backward_kernel(const int* __restrict__ win, const float* __restrict__ gL, float* __restrict__ gx, long N, long F, int ntile, int C,
                                int hop) {
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    float* gb = gx + (size_t)b * C * N;
    const int* wb = win + (size_t)b * F;
    const float* lb = gL + (size_t)b * F;
    const int lh = 31 - __builtin_clz(hop);
#pragma unroll 4
    for (int k = 0; k < BL_SPT; ++k) {
        const long m = (long)tile * BL_TILE + tid + BL_THREADS * k;
        if (m >= N) break;
        const long j = (m + hop - 1) >> lh;
        const int w = wb[j];
        const int pos = m ? (int)((m - 1) & (hop - 1)) : 0, s = (w >> 11) & 3;
        const bool here = (w & 2047) == pos;
        const int cw = w >> 13;
        const float g = lb[j];
        const float v = s == 1 ? g : (s == 2 ? -g : (s == 3 ? __builtin_nanf("") : 0.f * g));
        for (int c = 0; c < C; ++c) gb[(size_t)c * N + m] = here && c == cw ? v : 0.f;
    }
}

__global__ void __launch_bounds__(BL_THREADS)
blocklevel_power_backward_kernel(const float* __restrict__ x, const float* __restrict__ gL, float* __restrict__ gx, long N, long F, int ntile, int C,
                                 int hop) {
    const int tid = threadIdx.x, b = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const float* xb = x + (size_t)b * C * N;
    float* gb = gx + (size_t)b * C * N;
    const float* lb = gL + (size_t)b * F;
    const int lh = 31 - __builtin_clz(hop);
    const float two_c = 2.f * (1.f / (float)C), invh = 1.f / (float)hop;
#pragma unroll 4
    for (int k = 0; k < BL_SPT; ++k) {
        const long m = (long)tile * BL_TILE + tid + BL_THREADS * k;
        if (m >= N) break;
        const long j = (m + hop - 1) >> lh;
        const float g = two_c * (m ? invh : 1.f) * lb[j];
        for (int c = 0; c < C; ++c) gb[(size_t)c * N + m] = g * xb[(size_t)c * N + m];
    }
}

// ---- ballistics -------------------------------------------------------------------------------------------------------------------------
struct BalCoef { double c, t; bool clamped, nan; };
__device__ __forceinline__ BalCoef bal_coef(const float* __restrict__ ctl, int b, int hop, double sr) {
    const double r = (double)ctl[b];
    BalCoef k;
    k.nan = r != r;
    k.clamped = r < 0.1 || r > 10000.0;
    k.t = r < 0.1 ? 0.1 : (r > 10000.0 ? 10000.0 : r);                       // a NaN stays
    k.c = -expm1(-2.1972245773362196 * (double)hop / (sr * k.t / 1000.0));
    return k;
}

__global__ void __launch_bounds__(64)
ballistics_forward_kernel(const float* __restrict__ P, const float* __restrict__ att, const float* __restrict__ rel, float* __restrict__ E,
                          unsigned char* __restrict__ up, long F, int hop, double sr) {
#pragma clang fp contract(off)
    __shared__ float sP[BAL_CHUNK], sE[BAL_CHUNK];
    __shared__ unsigned char sM[BAL_CHUNK];
    const int lane = threadIdx.x, b = blockIdx.x;
    const BalCoef ka = bal_coef(att, b, hop, sr), kr = bal_coef(rel, b, hop, sr);
    const float pois = ka.nan || kr.nan ? __builtin_nanf("") : 0.f;
    const double ca = ka.c, cr = kr.c;
    const float* Pb = P + (size_t)b * F;
    float* Eb = E + (size_t)b * F;
    unsigned char* ub = up ? up + (size_t)b * F : nullptr;
    double e = 0.0;
    float nxt[BAL_PER];
#pragma unroll
    for (int m = 0; m < BAL_PER; ++m) {
        const long j = lane + 64 * m;
        nxt[m] = j < F ? Pb[j] : 0.f;
    }
    for (long k0 = 0; k0 < F; k0 += BAL_CHUNK) {
#pragma unroll
        for (int m = 0; m < BAL_PER; ++m) sP[lane + 64 * m] = nxt[m];
        if (k0 + BAL_CHUNK < F) {                                          // the next chunk's loads fly while this one is walked
#pragma unroll
            for (int m = 0; m < BAL_PER; ++m) {
                const long j = k0 + BAL_CHUNK + lane + 64 * m;
                nxt[m] = j < F ? Pb[j] : 0.f;
            }
        }
        __syncthreads();
        const int n = (int)(F - k0 < BAL_CHUNK ? F - k0 : BAL_CHUNK);
        if (lane == 0) {
#pragma unroll 8
            for (int i = 0; i < n; ++i) {
                const double p = (double)sP[i];
                const bool u = p > e;
                const double c = u ? ca : cr;
                e = e + c * (p - e);
                sE[i] = (float)e + pois;
                sM[i] = u ? 1 : 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < BAL_PER; ++m) {
            const int i = lane + 64 * m;
            if (i < n) {
                Eb[k0 + i] = sE[i];
                if (ub) ub[k0 + i] = sM[i];
            }
        }
        __syncthreads();
    }
}

// gP, gatt, grel: each may be null
__global__ void __launch_bounds__(64)
ballistics_backward_kernel(const float* __restrict__ P, const float* __restrict__ att, const float* __restrict__ rel, const float* __restrict__ E,
                           const unsigned char* __restrict__ up, const float* __restrict__ gE, float* __restrict__ gP, float* __restrict__ gatt,
                           float* __restrict__ grel, long F, int hop, double sr) {
#pragma clang fp contract(off)
    __shared__ double sD[BAL_CHUNK];
    __shared__ float sG[BAL_CHUNK], sO[BAL_CHUNK];
    __shared__ unsigned char sM[BAL_CHUNK];
    const int lane = threadIdx.x, b = blockIdx.x;
    const BalCoef ka = bal_coef(att, b, hop, sr), kr = bal_coef(rel, b, hop, sr);
    const float pois = ka.nan || kr.nan ? __builtin_nanf("") : 0.f;
    const double ca = ka.c, cr = kr.c, na = 1.0 - ka.c, nr = 1.0 - kr.c;
    const float* Pb = P + (size_t)b * F;
    const float* Eb = E + (size_t)b * F;
    const float* gb = gE + (size_t)b * F;
    const unsigned char* ub = up + (size_t)b * F;
    float* ob = gP ? gP + (size_t)b * F : nullptr;
    const bool sums = gatt || grel;
    double carry = 0.0, sum_a = 0.0, sum_r = 0.0;                              // carry = (1 - c_{j+1}) Lambda_{j+1}
    const long nchunk = (F + BAL_CHUNK - 1) / BAL_CHUNK;
    for (long q = nchunk - 1; q >= 0; --q) {
        const long k0 = q * BAL_CHUNK;
        const int n = (int)(F - k0 < BAL_CHUNK ? F - k0 : BAL_CHUNK);
#pragma unroll
        for (int m = 0; m < BAL_PER; ++m) {
            const int i = lane + 64 * m;
            const long j = k0 + i;
            const bool live = i < n;
            sG[i] = live ? gb[j] : 0.f;
            sM[i] = live ? ub[j] : 0;
            if (sums) sD[i] = live ? (double)Pb[j] - (j ? (double)Eb[j - 1] : 0.0) : 0.0;        // P_j - E_{j-1} from the saved float32 E, exact
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll 8
            for (int i = n - 1; i >= 0; --i) {
                const bool u = sM[i] != 0;
                const double lam = (double)sG[i] + carry;
                carry = (u ? na : nr) * lam;
                sO[i] = (float)((u ? ca : cr) * lam) + pois;
                if (sums) {
                    const double d = lam * sD[i];
                    sum_a = sum_a + (u ? d : 0.0);
                    sum_r = sum_r + (u ? 0.0 : d);
                }
            }
        }
        __syncthreads();
        if (ob) {
#pragma unroll
            for (int m = 0; m < BAL_PER; ++m) {
                const int i = lane + 64 * m;
                if (i < n) ob[k0 + i] = sO[i];
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        const double k = -2.1972245773362196 * (double)hop * 1000.0 / sr;
        if (gatt) gatt[b] = (ka.clamped ? 0.f : (float)(na * k / (ka.t * ka.t) * sum_a)) + pois;
        if (grel) grel[b] = (kr.clamped ? 0.f : (float)(nr * k / (kr.t * kr.t) * sum_r)) + pois;
    }
}

}  // namespace dasp

// ================================================================================================
// C-ABI (include/dasp_hip.h)
using namespace dasp;

namespace {
int bl_args(int B, int C, long N, int hop, int detector) {
    if (B <= 0 || C <= 0 || N <= 0 || hop <= 0 || detector < 0 || detector > 1) return DASP_ERR_ARG;
    if (!bl_hop_ok(hop) || C > BL_MAX_CH) return DASP_ERR_UNSUPPORTED;
    const long ntile = (N + BL_TILE - 1) / BL_TILE + 1;
    if (N > (1L << 40) || (long)B * ntile >= 0x7fffffffL || (long)B * bl_frames(N, hop) >= (1L << 37)) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
int bal_args(int B, long F, int hop, double sr) {
    if (B <= 0 || F <= 0 || hop <= 0 || !(sr > 0.0 && sr - sr == 0.0)) return DASP_ERR_ARG;
    if (!bl_hop_ok(hop) || (long)B * F >= (1L << 37)) return DASP_ERR_UNSUPPORTED;
    return DASP_OK;
}
}  // namespace

extern "C" {

int dasp_ballistics_chunk(void) { return BAL_CHUNK; }

int dasp_blocklevel_forward(const float* x, float* level, int* winners, int B, int C, long N, int hop, int detector, void* stream) {
    if (!x || !level) return DASP_ERR_ARG;
    const int s = bl_args(B, C, N, hop, detector);
    if (s != DASP_OK) return s;
    const long F = bl_frames(N, hop);
    const int ntile = (int)(((F - 1) * hop + BL_TILE - 1) / BL_TILE);
    const dim3 grid((unsigned)(B * ntile)), block(BL_THREADS);
    if (detector == 0)
        hipLaunchKernelGGL(blocklevel_forward_kernel<true>, grid, block, 0, (hipStream_t)stream, x, level, winners, N, F, ntile, C, hop);
    else
        hipLaunchKernelGGL(blocklevel_forward_kernel<false>, grid, block, 0, (hipStream_t)stream, x, level, nullptr, N, F, ntile, C, hop);
    return launch_status();
}

int dasp_blocklevel_backward(const float* x, const int* winners, const float* glevel, float* gx, int B, int C, long N, int hop, int detector,
                             void* stream) {
    if (!glevel || !gx) return DASP_ERR_ARG;
    const int s = bl_args(B, C, N, hop, detector);
    if (s != DASP_OK) return s;
    if (detector == 0 ? !winners : !x) return DASP_ERR_ARG;
    const long F = bl_frames(N, hop);
    const int ntile = (int)((N + BL_TILE - 1) / BL_TILE);
    const dim3 grid((unsigned)(B * ntile)), block(BL_THREADS);
    if (detector == 0)
        hipLaunchKernelGGL(blocklevel_peak_backward_kernel, grid, block, 0, (hipStream_t)stream, winners, glevel, gx, N, F, ntile, C, hop);
    else
        hipLaunchKernelGGL(blocklevel_power_backward_kernel, grid, block, 0, (hipStream_t)stream, x, glevel, gx, N, F, ntile, C, hop);
    return launch_status();
}

int dasp_ballistics_forward(const float* curve, const float* attack_ms, const float* release_ms, float* out, unsigned char* up, int B, long F,
                            int hop, double sample_rate, void* stream) {
    if (!curve || !attack_ms || !release_ms || !out) return DASP_ERR_ARG;
    const int s = bal_args(B, F, hop, sample_rate);
    if (s != DASP_OK) return s;
    hipLaunchKernelGGL(ballistics_forward_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, curve, attack_ms, release_ms, out, up, F, hop,
                       sample_rate);
    return launch_status();
}

int dasp_ballistics_backward(const float* curve, const float* attack_ms, const float* release_ms, const float* out, const unsigned char* up,
                             const float* gout, float* gcurve, float* gattack, float* grelease, int B, long F, int hop, double sample_rate,
                             void* stream) {
    if (!curve || !attack_ms || !release_ms || !out || !up || !gout || (!gcurve && !gattack && !grelease)) return DASP_ERR_ARG;
    const int s = bal_args(B, F, hop, sample_rate);
    if (s != DASP_OK) return s;
    hipLaunchKernelGGL(ballistics_backward_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, curve, attack_ms, release_ms, out, up, gout,
                       gcurve, gattack, grelease, F, hop, sample_rate);
    return launch_status();
}

}  // extern "C"
