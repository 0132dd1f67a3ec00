// What the two swept state-variable filters share (tvfilter, tveq): the tile geometry, one sample of Simper's trapezoidal recurrence, the
// 2 x 2 affine map of a run of samples, the scan of those maps over a tile, the sum of an interval's lanes and the host's size helpers.
// Everything here was moved out of tvfilter.hip as it stood; that file's header comment describes the walk these pieces belong to.
#pragma once

#include "row_helpers.hpp"

namespace dasp {

constexpr int TV_THREADS = 256;
constexpr int TV_SPT = 8;                            // consecutive samples per thread
constexpr int TV_TILE = TV_THREADS * TV_SPT;
constexpr int TV_NW = TV_THREADS / 64;
constexpr int TV_STAGE = TV_TILE + TV_TILE / TV_SPT; // a staged tile: sample i at word i + i / 8
constexpr int TV_FP = TV_TILE / 8 + 1;               // frame points of a tile at the smallest hop
constexpr int TV_HOP_MIN = 8, TV_HOP_MAX = TV_TILE;

struct TvMap { float a, b, c, d, u, v; };             // z -> [[a, b], [c, d]] z + (u, v)

__device__ __forceinline__ double tv_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }   // a NaN stays

// The coefficients of a thread's 8 samples
struct TvRun { float g[TV_SPT], k[TV_SPT], a1[TV_SPT], a2[TV_SPT], a3[TV_SPT], t[TV_SPT]; };

// One sample of the filter: z = (z1, z2) before it, replaced by the state after it.
__device__ __forceinline__ void tv_step(float& z1, float& z2, float x, float a1, float a2, float a3, float& v1, float& v2) {
    const float v3 = x - z2;
    v1 = __builtin_fmaf(a1, z1, a2 * v3);
    v2 = z2 + __builtin_fmaf(a2, z1, a3 * v3);
    z1 = __builtin_fmaf(2.f, v1, -z1);
    z2 = __builtin_fmaf(2.f, v2, -z2);
}

__device__ __forceinline__ TvMap tv_after(const TvMap& L, const TvMap& E) {          // E first, then L
    TvMap r;
    r.a = __builtin_fmaf(L.a, E.a, L.b * E.c);
    r.b = __builtin_fmaf(L.a, E.b, L.b * E.d);
    r.c = __builtin_fmaf(L.c, E.a, L.d * E.c);
    r.d = __builtin_fmaf(L.c, E.b, L.d * E.d);
    r.u = __builtin_fmaf(L.a, E.u, __builtin_fmaf(L.b, E.v, L.u));
    r.v = __builtin_fmaf(L.c, E.u, __builtin_fmaf(L.d, E.v, L.v));
    return r;
}

// the map of the lane DPP names, or the identity
template <int CTRL, int ROW_MASK> __device__ __forceinline__ TvMap tv_dpp(const TvMap& m) {
    return TvMap{dpp_or_one<CTRL, ROW_MASK>(m.a), dpp_or_zero<CTRL, ROW_MASK>(m.b), dpp_or_zero<CTRL, ROW_MASK>(m.c), dpp_or_one<CTRL, ROW_MASK>(m.d),
                 dpp_or_zero<CTRL, ROW_MASK>(m.u), dpp_or_zero<CTRL, ROW_MASK>(m.v)};
}

// The scan of the runs' maps. run: the thread's map; (c1, c2): the state before the tile; wt: six floats per wave. Returns in (o1, o2)
// the state before the thread's first sample. One barrier; wt is free again after the caller's next one.
__device__ __forceinline__ void tv_scan(const TvMap& run, float c1, float c2, float* wt, float& o1, float& o2) {
    const int lane = lane_id(), wv = wave_id();
    TvMap agg = run;
    agg = tv_after(agg, tv_dpp<0x111, 0xf>(agg));       // row_shr:1
    agg = tv_after(agg, tv_dpp<0x112, 0xf>(agg));       // row_shr:2
    agg = tv_after(agg, tv_dpp<0x114, 0xf>(agg));       // row_shr:4
    agg = tv_after(agg, tv_dpp<0x118, 0xf>(agg));       // row_shr:8
    agg = tv_after(agg, tv_dpp<0x142, 0xa>(agg));       // row_bcast:15   rows 1, 3 after the row before them
    agg = tv_after(agg, tv_dpp<0x143, 0xc>(agg));       // row_bcast:31   rows 2, 3 after rows 0..1
    TvMap ex{shift_up(agg.a, 1), shift_up(agg.b, 1), shift_up(agg.c, 1), shift_up(agg.d, 1), shift_up(agg.u, 1), shift_up(agg.v, 1)};
    if (lane == 0) ex = TvMap{1.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    if (lane == 63) {
        float* w = wt + 6 * wv;
        w[0] = agg.a; w[1] = agg.b; w[2] = agg.c; w[3] = agg.d; w[4] = agg.u; w[5] = agg.v;
    }
    lds_barrier();
    for (int u = 0; u < wv; ++u) {                      // the state before the wave's first sample
        const float* w = wt + 6 * u;
        const float n1 = __builtin_fmaf(w[0], c1, __builtin_fmaf(w[1], c2, w[4]));
        const float n2 = __builtin_fmaf(w[2], c1, __builtin_fmaf(w[3], c2, w[5]));
        c1 = n1;
        c2 = n2;
    }
    o1 = __builtin_fmaf(ex.a, c1, __builtin_fmaf(ex.b, c2, ex.u));
    o2 = __builtin_fmaf(ex.c, c1, __builtin_fmaf(ex.d, c2, ex.v));
}

// The map of a run in forward time: from the two unit states without input, and from zero state with the run's x.
__device__ __forceinline__ TvMap tv_run_map(const float (&x)[TV_SPT], const TvRun& c) {
    float e1 = 1.f, e2 = 0.f, f1 = 0.f, f2 = 1.f, z1 = 0.f, z2 = 0.f, v1, v2;
#pragma unroll
    for (int j = 0; j < TV_SPT; ++j) {
        tv_step(e1, e2, 0.f, c.a1[j], c.a2[j], c.a3[j], v1, v2);
        tv_step(f1, f2, 0.f, c.a1[j], c.a2[j], c.a3[j], v1, v2);
        tv_step(z1, z2, x[j], c.a1[j], c.a2[j], c.a3[j], v1, v2);
    }
    return TvMap{e1, f1, e2, f2, z1, z2};
}

// the runs of an interval: the lanes of a group of W by an xor butterfly, every lane of it ending with the same bits
template <int K> __device__ __forceinline__ void tv_group_sum(double (&d)[K], int W) {
    for (int s = 1; s < W; s <<= 1) {
#pragma unroll
        for (int i = 0; i < K; ++i) d[i] += __shfl_xor(d[i], s, 64);
    }
}

inline long tv_ntile(long N) { return (N + TV_TILE - 1) / TV_TILE; }
inline bool tv_hop_pow2(int hop) { return hop > 0 && (hop & (hop - 1)) == 0; }
inline bool tv_hop_ok(int hop) { return tv_hop_pow2(hop) && hop >= TV_HOP_MIN && hop <= TV_HOP_MAX; }
inline long tv_frames_of(long N, int hop) { return (N + hop - 1) / hop + 1; }

}  // namespace dasp
