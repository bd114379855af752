// What the dual-tree kernels of dtcwt.hip, scat.hip and dtcwt_loss.hip share: tap structs, tile constants, the extension's index
// map, q2c / c2q, the four tile bodies (level 1 and level >= 2, forward and inverse) that every one of those kernels runs, and the
// host-side argument checks, tile counts and synthesis tap table.  Notation and index maps: the head of dtcwt.hip.
#pragma once
#include <cstdint>
#include <type_traits>
#include "common.h"

namespace faoctasr {

constexpr int DT_MAXL = 20;                       // level 1: odd 3..19; q-shift: even 4..20
constexpr float DT_S = 0.70710678118654752440f;

struct DtStr { long n, c, o, r, w, i; };         // bandpass element strides
struct DtLow { long n, c, r; };                  // lowpass input element strides

struct DtTaps1 { float f0[DT_MAXL], f1[DT_MAXL]; };                      // level 1: lowpass, highpass
struct DtTaps2 { float lo0[DT_MAXL], lo1[DT_MAXL], hi0[DT_MAXL], hi1[DT_MAXL]; };   // level >= 2 analysis, by output phase
struct DtTapsI { float lo[4][DT_MAXL / 2], hi[4][DT_MAXL / 2]; int dlo[4], dhi[4]; };   // level >= 2 synthesis, by output phase q
// the three-filter (rotationally symmetric) banks, an entry point's optional third filter: the two-filter taps and the bandpass filter of the diagonal band hh
struct DtTaps1R : DtTaps1 { float f2[DT_MAXL]; int L2; };               // level 1: + bandpass, of its own odd length
struct DtTaps2R : DtTaps2 { float ba0[DT_MAXL], ba1[DT_MAXL]; };        // level >= 2 analysis: + the bandpass pair, phased as hi0, hi1
struct DtTapsIR : DtTapsI { float ba[4][DT_MAXL / 2]; int dba[4]; };    // level >= 2 synthesis: + a third (highpass-call) table
// the tap structs of a kernel's two-filter (BP = false) and three-filter (BP = true) form
template <bool BP> struct DtBank { using T1 = DtTaps1; using T2 = DtTaps2; using TI = DtTapsI; };
template <> struct DtBank<true> { using T1 = DtTaps1R; using T2 = DtTaps2R; using TI = DtTapsIR; };

// level-1 tiles (forward: of ll; inverse: of y) and the level >= 2 ones (forward: of ll = 4 x 32 quads; inverse: of y)
constexpr int J1_TH = 16, J1_TW = 64, J1_PR = J1_TH + DT_MAXL - 2, J1_PC = J1_TW + DT_MAXL - 2;          // halo 2 * 9
constexpr int F2_TH = 8, F2_TW = 64, F2_PR = 2 * F2_TH + 2 * DT_MAXL - 4, F2_PC = 2 * F2_TW + 2 * DT_MAXL - 4;
constexpr int I2_TH = 32, I2_TW = 64, I2_PR = I2_TH / 2 + DT_MAXL, I2_PC = I2_TW / 2 + DT_MAXL;

// level-1 halo: the largest half-length of the bank's filters
template <bool BP>
__device__ __forceinline__ int dt_halo1(int L0, int L1, const typename DtBank<BP>::T1& taps) {
    int L = L0 > L1 ? L0 : L1;
    if constexpr (BP) L = taps.L2 > L ? taps.L2 : L;
    return L >> 1;
}

// index of the sample that position j of the extension reads; -1 for a zero
__device__ __forceinline__ int dt_map(int j, int N, int sym) {
    if (sym) {
        int m = j % (2 * N);
        if (m < 0) m += 2 * N;
        return m < N ? m : 2 * N - 1 - m;
    }
    return (j >= 0 && j < N) ? j : -1;
}

__device__ __forceinline__ void dt_put(float* p, long si, bool vec, float re, float im) {
    if (vec) *reinterpret_cast<float2*>(p) = make_float2(re, im);
    else { p[0] = re; p[si] = im; }
}

// q2c of one quad (top = a, b; bot = c, d): z1 = (a - d) + i (b + c), z2 = (a + d) + i (b - c), scaled by 1/sqrt 2 first
__device__ __forceinline__ void dt_q2c_val(float2 top, float2 bot, float2* z1, float2* z2) {
    const float a = top.x * DT_S, b = top.y * DT_S, c = bot.x * DT_S, d = bot.y * DT_S;
    *z1 = make_float2(a - d, b + c);
    *z2 = make_float2(a + d, b - c);
}

// q2c of one quad into orientations o1 (z1) and o2 (z2)
__device__ __forceinline__ void dt_q2c(float* q, const DtStr& s, bool vec, int o1, int o2, float2 top, float2 bot) {
    float2 z1, z2;
    dt_q2c_val(top, bot, &z1, &z2);
    dt_put(q + o1 * s.o, s.i, vec, z1.x, z1.y);
    dt_put(q + o2 * s.o, s.i, vec, z2.x, z2.y);
}

// c2q: the value at row parity pr, column parity pc of the quad whose complex pair has the components w1, w2 that the parities
// select ((0,1) and (1,0) take the imaginary parts, the other two the real ones)
__device__ __forceinline__ float dt_c2q_val(float w1, float w2, int pr, int pc) {
    return (pr ? (pc ? w2 - w1 : w1 - w2) : w1 + w2) * DT_S;
}

// c2q: the value at row parity pr, column parity pc of the quad whose complex pair (w1, w2) starts at p1, p2
__device__ __forceinline__ float dt_c2q(const float* p1, const float* p2, long si, int pr, int pc) {
    const long comp = (pr ^ pc) ? si : 0;                   // (0,1) and (1,0) read the imaginary parts
    return dt_c2q_val(p1[comp], p2[comp], pr, pc);
}

// stage one coefficient position (sr, sc) of the four full-resolution planes ll, lh, hl, hh (c2q applied on the way)
__device__ __forceinline__ void dt_stage(const float* lp, DtLow ls, const float* hp, const DtStr& hs, int sr, int sc, float* o0, float* o1,
                                         float* o2, float* o3) {
    *o0 = lp ? lp[sr * ls.r + sc] : 0.f;
    if (hp) {
        const float* q = hp + (long)(sr >> 1) * hs.r + (long)(sc >> 1) * hs.w;
        const int pr = sr & 1, pc = sc & 1;
        *o1 = dt_c2q(q, q + 5 * hs.o, hs.i, pr, pc);                      // lh: 15, 165
        *o2 = dt_c2q(q + 2 * hs.o, q + 3 * hs.o, hs.i, pr, pc);           // hl: 75, 105
        *o3 = dt_c2q(q + hs.o, q + 4 * hs.o, hs.i, pr, pc);               // hh: 45, 135
    } else {
        *o1 = *o2 = *o3 = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The tile bodies.  A kernel decodes its block (dt_tile), calls a body on LDS arrays that it declares itself -- an array a form
// never touches (mid_hi of the lowpass-only forward, mid_ba of the two-filter banks) is one dummy row and costs no LDS -- and
// does its own pointwise part.  256 threads.  Every sum is one fmaf chain in the order t = 0 .. L-1.
// ---------------------------------------------------------------------------------------------------------------------------
struct DtTile { int tw, th; long plane; };
__device__ __forceinline__ DtTile dt_tile(int tiles_h, int tiles_w) {
    int b = blockIdx.x;
    DtTile t;
    t.tw = b % tiles_w; b /= tiles_w;
    t.th = b % tiles_h;
    t.plane = b / tiles_h;
    return t;
}

// level-1 geometry: the halo hm, the offsets of the three filters into it, the patch's extent (<= J1_PR, J1_PC)
struct DtGeo1 { int hm, a0, a1, a2, rows, cols; };
template <bool BP>
__device__ __forceinline__ DtGeo1 dt_geo1(int L0, int L1, const typename DtBank<BP>::T1& taps) {
    const int hm = dt_halo1<BP>(L0, L1, taps);
    int a2 = 0;
    if constexpr (BP) a2 = hm - (taps.L2 >> 1);
    return {hm, hm - (L0 >> 1), hm - (L1 >> 1), a2, J1_TH + 2 * hm, J1_TW + 2 * hm};
}

// Level 1 forward, first half: stage the patch of the tile at (oi0, oj0) of the plane xp (row stride xr) and run the W pass into
// mid_*.  Ends on a barrier; every thread of the block calls it, and a caller that loops over planes calls it again only from
// threads that are all past dt_fwd1_quad (its first barrier then separates their reads of mid_* from the next W pass).
template <bool HIGHS, bool BP>
__device__ __forceinline__ void dt_fwd1_rows(const float* xp, long xr, int oi0, int oj0, int H, int W, int sym, int L0, int L1,
                                             const typename DtBank<BP>::T1& taps, float (*patch)[J1_PC], float (*mid_lo)[J1_TW],
                                             float (*mid_hi)[J1_TW], float (*mid_ba)[J1_TW]) {
    const int tid = threadIdx.x;
    const DtGeo1 g = dt_geo1<BP>(L0, L1, taps);
    for (int r = tid >> 6; r < g.rows; r += 4) {
        const int sr = dt_map(oi0 - g.hm + r, H, sym);
        for (int cc = tid & 63; cc < g.cols; cc += 64) {
            const int sc = dt_map(oj0 - g.hm + cc, W, sym);
            patch[r][cc] = (sr >= 0 && sc >= 0) ? xp[sr * xr + sc] : 0.f;
        }
    }
    __syncthreads();

    const int cc = tid & 63;                                              // W pass: thread (r, cc) filters patch row r at tile column cc
    for (int r = tid >> 6; r < g.rows; r += 4) {
        float lo = 0.f, hv = 0.f;
        for (int t = 0; t < L0; ++t) lo = fmaf(taps.f0[t], patch[r][cc + t + g.a0], lo);
        if constexpr (HIGHS)
            for (int t = 0; t < L1; ++t) hv = fmaf(taps.f1[t], patch[r][cc + t + g.a1], hv);
        mid_lo[r][cc] = lo;
        if constexpr (HIGHS) mid_hi[r][cc] = hv;
        if constexpr (BP) {
            float bv = 0.f;
            for (int t = 0; t < taps.L2; ++t) bv = fmaf(taps.f2[t], patch[r][cc + t + g.a2], bv);
            mid_ba[r][cc] = bv;
        }
    }
    __syncthreads();
}

// Level 1 forward, second half: the H pass of the 2x2 quad (qi, qj) of the tile (8 x 32 quads, a thread each), column pairs read
// as float2.  Rows 0 and 1 of the quad in ll, lh, hl, hh (the last three only with HIGHS).  BP: hh = col(ba, h2)
struct DtQuad1 { float2 ll[2], lh[2], hl[2], hh[2]; };
template <bool HIGHS, bool BP>
__device__ __forceinline__ DtQuad1 dt_fwd1_quad(int qi, int qj, int L0, int L1, const typename DtBank<BP>::T1& taps,
                                                const float (*mid_lo)[J1_TW], const float (*mid_hi)[J1_TW], const float (*mid_ba)[J1_TW]) {
    const DtGeo1 g = dt_geo1<BP>(L0, L1, taps);
    DtQuad1 o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        float2 s = make_float2(0.f, 0.f), u = s, p = s, q = s;
        for (int t = 0; t < L0; ++t) {
            const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + g.a0][2 * qj]);
            s.x = fmaf(taps.f0[t], v.x, s.x); s.y = fmaf(taps.f0[t], v.y, s.y);
            if constexpr (HIGHS) {
                const float2 w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + g.a0][2 * qj]);
                p.x = fmaf(taps.f0[t], w.x, p.x); p.y = fmaf(taps.f0[t], w.y, p.y);
            }
        }
        if constexpr (HIGHS) {
            for (int t = 0; t < L1; ++t) {
                const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + g.a1][2 * qj]);
                u.x = fmaf(taps.f1[t], v.x, u.x); u.y = fmaf(taps.f1[t], v.y, u.y);
                if constexpr (!BP) {
                    const float2 w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + g.a1][2 * qj]);
                    q.x = fmaf(taps.f1[t], w.x, q.x); q.y = fmaf(taps.f1[t], w.y, q.y);
                }
            }
        }
        if constexpr (BP) {
            for (int t = 0; t < taps.L2; ++t) {
                const float2 w = *reinterpret_cast<const float2*>(&mid_ba[2 * qi + d + t + g.a2][2 * qj]);
                q.x = fmaf(taps.f2[t], w.x, q.x); q.y = fmaf(taps.f2[t], w.y, q.y);
            }
        }
        o.ll[d] = s; o.lh[d] = u; o.hl[d] = p; o.hh[d] = q;
    }
    return o;
}

// Level >= 2 forward, first half: stage the patch of the tile whose first quad is (i0, j0) -- patch (r, cc) is x position
// 4 i0 + 2 - m + r, 2 F2_TH + 2 m - 4 rows (<= F2_PR) -- and run the W pass.  Barriers and callers as dt_fwd1_rows.
template <bool HIGHS, bool BP>
__device__ __forceinline__ void dt_fwd2_rows(const float* xp, long xr, int i0, int j0, int H, int W, int m,
                                             const typename DtBank<BP>::T2& taps, float (*patch)[F2_PC], float (*mid_lo)[F2_TW],
                                             float (*mid_hi)[F2_TW], float (*mid_ba)[F2_TW]) {
    const int tid = threadIdx.x;
    const int rows = 2 * F2_TH + 2 * m - 4, cols = 2 * F2_TW + 2 * m - 4;
    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(4 * i0 + 2 - m + r, H, 1);
        for (int cc = tid & 63; cc < cols; cc += 64)
            patch[r][cc] = xp[sr * xr + dt_map(4 * j0 + 2 - m + cc, W, 1)];
    }
    __syncthreads();

    // W pass: tile column cc = 2 i + p; the float2 at patch column 4 i + 2 t holds the samples at offsets 2 - m and 3 - m
    const int cc = tid & 63, i = cc >> 1, p = cc & 1;
    for (int r = tid >> 6; r < rows; r += 4) {
        float lo = 0.f, hv = 0.f, bv = 0.f;
        for (int t = 0; t < m; ++t) {
            const float2 v = *reinterpret_cast<const float2*>(&patch[r][4 * i + 2 * t]);
            lo = fmaf(p ? taps.lo1[t] : taps.lo0[t], p ? v.y : v.x, lo);
            if constexpr (HIGHS) hv = fmaf(p ? taps.hi1[t] : taps.hi0[t], p ? v.x : v.y, hv);
            if constexpr (BP) bv = fmaf(p ? taps.ba1[t] : taps.ba0[t], p ? v.x : v.y, bv);
        }
        mid_lo[r][cc] = lo;
        if constexpr (HIGHS) mid_hi[r][cc] = hv;
        if constexpr (BP) mid_ba[r][cc] = bv;
    }
    __syncthreads();
}

// Level >= 2 forward, second half: the H pass of quad (qi, qj) of the tile (4 x 32 quads) on one of two paths, threads 0..127 on
// the W-lowpass plane (path 0: l = ll, h = lh), threads 128..255 on the W-highpass plane (path 1: l = hl, h = hh; BP: hh from the
// W-bandpass plane on the bandpass taps).  l0, l1: rows 2 qi, 2 qi + 1 of the lowpass call; h0, h1: of the highpass call.
// The lowpass-only form has path 0 alone.
struct DtQuad2 { float2 l0, l1, h0, h1; };
template <bool HIGHS, bool BP>
__device__ __forceinline__ DtQuad2 dt_fwd2_quad(int path, int qi, int qj, int m, const typename DtBank<BP>::T2& taps,
                                                const float (*mid_lo)[F2_TW], const float (*mid_hi)[F2_TW], const float (*mid_ba)[F2_TW]) {
    DtQuad2 o;
    o.l0 = o.l1 = o.h0 = o.h1 = make_float2(0.f, 0.f);
    for (int t = 0; t < m; ++t) {
        const float* mp = &mid_lo[4 * qi + 2 * t][2 * qj];
        if constexpr (HIGHS) mp = path ? &mid_hi[4 * qi + 2 * t][2 * qj] : mp;
        const float2 r0 = *reinterpret_cast<const float2*>(mp), r1 = *reinterpret_cast<const float2*>(mp + F2_TW);
        o.l0.x = fmaf(taps.lo0[t], r0.x, o.l0.x); o.l0.y = fmaf(taps.lo0[t], r0.y, o.l0.y);
        o.l1.x = fmaf(taps.lo1[t], r1.x, o.l1.x); o.l1.y = fmaf(taps.lo1[t], r1.y, o.l1.y);
        if constexpr (BP) {
            const float* bp = path ? &mid_ba[4 * qi + 2 * t][2 * qj] : mp;
            const float2 b0 = *reinterpret_cast<const float2*>(bp), b1 = *reinterpret_cast<const float2*>(bp + F2_TW);
            const float k0 = path ? taps.ba0[t] : taps.hi0[t], k1 = path ? taps.ba1[t] : taps.hi1[t];
            o.h0.x = fmaf(k0, b1.x, o.h0.x); o.h0.y = fmaf(k0, b1.y, o.h0.y);
            o.h1.x = fmaf(k1, b0.x, o.h1.x); o.h1.y = fmaf(k1, b0.y, o.h1.y);
        } else if constexpr (HIGHS) {
            o.h0.x = fmaf(taps.hi0[t], r1.x, o.h0.x); o.h0.y = fmaf(taps.hi0[t], r1.y, o.h0.y);
            o.h1.x = fmaf(taps.hi1[t], r0.x, o.h1.x); o.h1.y = fmaf(taps.hi1[t], r0.y, o.h1.y);
        }
    }
    return o;
}

// Level 1 inverse of the tile at (t0, s0) into the plane yp [H, W].  stage(sr, sc, &ll, &lh, &hl, &hh) writes coefficient position
// (sr, sc) of the four full-resolution planes; has_lo / has_hi say whether ll / the three bands are there at all (their sums are
// skipped otherwise; a caller that passes `true` compiles without the tests).
//   H pass: lo = col(lh, g1) + col(ll, g0), hi = col(hh, g1) + col(hl, g0);   BP: hi = col(hl, g0), ba = col(hh, g2)
//   W pass: y = row(hi, g1) + row(lo, g0);                                    BP: (row(hi, g1) + row(lo, g0)) + row(ba, g2)
template <bool BP, class Stage>
__device__ __forceinline__ void dt_inv1(Stage stage, bool has_lo, bool has_hi, float* yp, int t0, int s0, int H, int W, int sym, int L0,
                                        int L1, const typename DtBank<BP>::T1& taps, float (*cf)[J1_PR][J1_PC], float (*mid_lo)[J1_PC],
                                        float (*mid_hi)[J1_PC], float (*mid_ba)[J1_PC]) {
    const int tid = threadIdx.x;
    const DtGeo1 g = dt_geo1<BP>(L0, L1, taps);
    for (int r = tid >> 6; r < g.rows; r += 4) {
        const int sr = dt_map(t0 - g.hm + r, H, sym);
        for (int cc = tid & 63; cc < g.cols; cc += 64) {
            const int sc = dt_map(s0 - g.hm + cc, W, sym);
            if (sr >= 0 && sc >= 0) stage(sr, sc, &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
            else cf[0][r][cc] = cf[1][r][cc] = cf[2][r][cc] = cf[3][r][cc] = 0.f;
        }
    }
    __syncthreads();

    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {                        // H pass: every tile row and patch column
        for (int cc = tid & 63; cc < g.cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            if (has_hi)
                for (int t = 0; t < L1; ++t) {
                    l1 = fmaf(taps.f1[t], cf[1][tt + t + g.a1][cc], l1);
                    if constexpr (!BP) h1 = fmaf(taps.f1[t], cf[3][tt + t + g.a1][cc], h1);
                }
            const auto col0 = [&](auto hi, auto lo) {                      // one loop for what is there, no test inside it
                for (int t = 0; t < L0; ++t) {
                    if constexpr (hi) h0 = fmaf(taps.f0[t], cf[2][tt + t + g.a0][cc], h0);
                    if constexpr (lo) l0 = fmaf(taps.f0[t], cf[0][tt + t + g.a0][cc], l0);
                }
            };
            if (has_hi && has_lo) col0(std::true_type{}, std::true_type{});
            else if (has_hi) col0(std::true_type{}, std::false_type{});
            else col0(std::false_type{}, std::true_type{});
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) {
                if (has_hi)
                    for (int t = 0; t < taps.L2; ++t) h1 = fmaf(taps.f2[t], cf[3][tt + t + g.a2][cc], h1);
                mid_hi[tt][cc] = h0;
                mid_ba[tt][cc] = h1;
            } else {
                mid_hi[tt][cc] = h1 + h0;
            }
        }
    }
    __syncthreads();

    const int ss = tid & 63, s = s0 + ss;
    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= H || s >= W) continue;
        float vh = 0.f, vl = 0.f;
        if (has_hi)
            for (int k = 0; k < L1; ++k) vh = fmaf(taps.f1[k], mid_hi[tt][ss + k + g.a1], vh);
        for (int k = 0; k < L0; ++k) vl = fmaf(taps.f0[k], mid_lo[tt][ss + k + g.a0], vl);
        if constexpr (BP) {
            float vb = 0.f;
            if (has_hi)
                for (int k = 0; k < taps.L2; ++k) vb = fmaf(taps.f2[k], mid_ba[tt][ss + k + g.a2], vb);
            yp[(long)t * W + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * W + s] = vh + vl;
        }
    }
}

// Level >= 2 inverse of the tile at (t0, s0), multiples of 4, into the plane yp [2R, 2Q]; stage, has_lo, has_hi and the sums as
// dt_inv1, always symmetric.  Patch (r, cc) is coefficient position 2 (t0 / 4) - m2 + r.  tl / td: the per-phase taps and offsets
// in LDS, for the lane-varying phase of the W pass (lowpass call, highpass call; BP: and the bandpass one).
template <bool BP, class Stage>
__device__ __forceinline__ void dt_inv2(Stage stage, bool has_lo, bool has_hi, float* yp, int t0, int s0, int R, int Q, int m2,
                                        const typename DtBank<BP>::TI& taps, float (*cf)[I2_PR][I2_PC], float (*mid_lo)[I2_PC],
                                        float (*mid_hi)[I2_PC], float (*mid_ba)[I2_PC], float (*tl)[4][DT_MAXL / 2], int (*td)[4]) {
    const int tid = threadIdx.x;
    const int OH = 2 * R, OW = 2 * Q, i0 = t0 >> 2, j0 = s0 >> 2;
    const int rows = I2_TH / 2 + 2 * m2, cols = I2_TW / 2 + 2 * m2;
    if (tid < 4 * (DT_MAXL / 2)) {
        tl[0][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.lo[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
        tl[1][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.hi[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
        if constexpr (BP) tl[2][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.ba[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
    }
    if (tid < 4) {
        td[0][tid] = taps.dlo[tid]; td[1][tid] = taps.dhi[tid];
        if constexpr (BP) td[2][tid] = taps.dba[tid];
    }
    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(2 * i0 - m2 + r, R, 1);
        for (int cc = tid & 63; cc < cols; cc += 64)
            stage(sr, dt_map(2 * j0 - m2 + cc, Q, 1), &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
    }
    __syncthreads();

    // H pass: a wave takes a tile row (its phase q is uniform), lanes the patch columns
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int q = tt & 3, ii = tt >> 2;                               // t0 is a multiple of 4
        const int rl = 2 * ii + td[0][q], rh = 2 * ii + td[1][q], rb = 2 * ii + td[BP ? 2 : 1][q];
        for (int cc = tid & 63; cc < cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            const auto col = [&](auto hi, auto lo) {                       // one loop for what is there, no test inside it
                for (int t = 0; t < m2; ++t) {
                    if constexpr (hi) {
                        l1 = fmaf(tl[1][q][t], cf[1][rh + 2 * t][cc], l1);
                        h1 = fmaf(tl[BP ? 2 : 1][q][t], cf[3][rb + 2 * t][cc], h1);     // BP: ba = col(hh, g2)
                        h0 = fmaf(tl[0][q][t], cf[2][rl + 2 * t][cc], h0);
                    }
                    if constexpr (lo) l0 = fmaf(tl[0][q][t], cf[0][rl + 2 * t][cc], l0);
                }
            };
            if (has_hi && has_lo) col(std::true_type{}, std::true_type{});
            else if (has_hi) col(std::true_type{}, std::false_type{});
            else col(std::false_type{}, std::true_type{});
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) { mid_hi[tt][cc] = h0; mid_ba[tt][cc] = h1; }
            else mid_hi[tt][cc] = h1 + h0;
        }
    }
    __syncthreads();

    const int ss = tid & 63, s = s0 + ss, q = ss & 3, jj = ss >> 2;
    const int cl = 2 * jj + td[0][q], ch = 2 * jj + td[1][q];
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= OH || s >= OW) continue;
        float vh = 0.f, vl = 0.f;
        if (has_hi)
            for (int k = 0; k < m2; ++k) vh = fmaf(tl[1][q][k], mid_hi[tt][ch + 2 * k], vh);
        for (int k = 0; k < m2; ++k) vl = fmaf(tl[0][q][k], mid_lo[tt][cl + 2 * k], vl);
        if constexpr (BP) {
            const int cb = 2 * jj + td[2][q];
            float vb = 0.f;
            if (has_hi)
                for (int k = 0; k < m2; ++k) vb = fmaf(tl[2][q][k], mid_ba[tt][cb + 2 * k], vb);
            yp[(long)t * OW + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * OW + s] = vh + vl;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
// shape check and tile counts of the level-1 kernels, the level >= 2 forwards and the level >= 2 inverses (H, W: of the result)
inline int dt_tiles1(const char* what, int H, int W, int* tiles_h, int* tiles_w) {
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be even and at least 2", what, H, W);
    *tiles_h = (H + J1_TH - 1) / J1_TH; *tiles_w = (W + J1_TW - 1) / J1_TW;
    return FAOCTASR_OK;
}
inline int dt_tiles2f(const char* what, int H, int W, int* tiles_h, int* tiles_w) {
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be multiples of 4", what, H, W);
    *tiles_h = (H / 2 + F2_TH - 1) / F2_TH; *tiles_w = (W / 2 + F2_TW - 1) / F2_TW;
    return FAOCTASR_OK;
}
inline int dt_tiles2i(const char* what, int H, int W, int* tiles_h, int* tiles_w) {
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: the result's H %d W %d must be multiples of 4", what, H, W);
    *tiles_h = (H + I2_TH - 1) / I2_TH; *tiles_w = (W + I2_TW - 1) / I2_TW;
    return FAOCTASR_OK;
}

inline int dt_blocks(const char* what, long N, int C, int tiles_h, int tiles_w, long* blocks) {
    if (N < 1 || C < 1) return fail(FAOCTASR_EINVAL, "%s: N %ld C %d", what, N, C);
    *blocks = N * C * tiles_h * (long)tiles_w;
    if (*blocks > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: N %ld C %d needs more than 2^31 - 1 blocks", what, N, C);
    return FAOCTASR_OK;
}

// The tap arguments of an entry point.  The third filter is optional -- NULL selects the two-filter form --; dt_with_taps* check
// the arguments, pack them once and hand run(form, taps) the struct of the form: (std::false_type, DtTaps1 / DtTaps2 / DtTapsI) or
// (std::true_type, DtTaps1R / DtTaps2R / DtTapsIR), the base part of the one packed struct or all of it.  Nothing here calls HIP.
template <class Run>
inline int dt_with_taps1(const char* what, const float* f0, int L0, const float* f1, int L1, const float* f2, int L2, Run run) {
    if (!f0 || !f1) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (L0 < 3 || L0 >= DT_MAXL || !(L0 & 1) || L1 < 3 || L1 >= DT_MAXL || !(L1 & 1))
        return fail(FAOCTASR_EINVAL, "%s: level-1 tap counts %d and %d must be odd and within 3..%d", what, L0, L1, DT_MAXL - 1);
    if (!f2 && L2 != 0) return fail(FAOCTASR_EINVAL, "%s: a NULL third filter takes the tap count 0, got %d", what, L2);
    if (f2 && (L2 < 3 || L2 >= DT_MAXL || !(L2 & 1)))
        return fail(FAOCTASR_EINVAL, "%s: level-1 third-filter tap count %d must be odd and within 3..%d", what, L2, DT_MAXL - 1);
    DtTaps1R t = {};
    for (int k = 0; k < L0; ++k) t.f0[k] = f0[k];
    for (int k = 0; k < L1; ++k) t.f1[k] = f1[k];
    if (!f2) return run(std::false_type{}, static_cast<const DtTaps1&>(t));
    for (int k = 0; k < L2; ++k) t.f2[k] = f2[k];
    t.L2 = L2;
    return run(std::true_type{}, t);
}

// the q-shift taps of both level >= 2 kinds: tree a and tree b of the lowpass, the highpass and the optional third pair
inline int dt_taps2_check(const char* what, const float* a0, const float* b0, const float* a1, const float* b1, const float* a2,
                          const float* b2, int m) {
    if (!a0 || !b0 || !a1 || !b1) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (m < 4 || m > DT_MAXL || (m & 1)) return fail(FAOCTASR_EINVAL, "%s: q-shift tap count %d must be even and within 4..%d", what, m, DT_MAXL);
    if (!a2 != !b2) return fail(FAOCTASR_EINVAL, "%s: the third filter pair (a2, b2) takes both pointers or two NULLs, got one", what);
    return FAOCTASR_OK;
}

// analysis taps by output phase: the lowpass call reads (h0b, h0a), the highpass calls (h1a, h1b) and (h2a, h2b)
template <class Run>
inline int dt_with_taps2(const char* what, const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                         const float* h2b, int m, Run run) {
    const int rc = dt_taps2_check(what, h0a, h0b, h1a, h1b, h2a, h2b, m);
    if (rc) return rc;
    DtTaps2R t = {};
    for (int k = 0; k < m; ++k) { t.lo0[k] = h0b[k]; t.lo1[k] = h0a[k]; t.hi0[k] = h1a[k]; t.hi1[k] = h1b[k]; }
    if (!h2a) return run(std::false_type{}, static_cast<const DtTaps2&>(t));
    for (int k = 0; k < m; ++k) { t.ba0[k] = h2a[k]; t.ba1[k] = h2b[k]; }
    return run(std::true_type{}, t);
}

// the table of lowlevel.py:154-239: per output phase q the polyphase half and offset of colifilt(X, fa, fb, highpass)
inline void dtcwt_ifilt_taps(const float* fa, const float* fb, int m, int highpass, float out[4][DT_MAXL / 2], int d[4]) {
    const int m2 = m / 2;
    // which filter (0 = fa, 1 = fb), which half (0 = even taps, 1 = odd taps), offset
    static const int even_lo[4][3] = {{0, 0, 0}, {1, 0, 1}, {0, 1, 2}, {1, 1, 3}}, even_hi[4][3] = {{0, 0, 1}, {1, 0, 0}, {0, 1, 3}, {1, 1, 2}};
    static const int odd_lo[4][3] = {{0, 1, 1}, {1, 1, 2}, {0, 0, 1}, {1, 0, 2}}, odd_hi[4][3] = {{0, 1, 2}, {1, 1, 1}, {0, 0, 2}, {1, 0, 1}};
    const int (*tab)[3] = (m2 & 1) ? (highpass ? odd_hi : odd_lo) : (highpass ? even_hi : even_lo);
    for (int q = 0; q < 4; ++q) {
        const float* f = tab[q][0] ? fb : fa;
        for (int t = 0; t < DT_MAXL / 2; ++t) out[q][t] = t < m2 ? f[2 * t + tab[q][1]] : 0.f;
        d[q] = tab[q][2];
    }
}

// synthesis tables: colifilt(X, g0b, g0a, False), colifilt(X, g1b, g1a, True) and, for hh, colifilt(X, g2b, g2a, True)
template <class Run>
inline int dt_with_tapsi(const char* what, const float* g0a, const float* g0b, const float* g1a, const float* g1b, const float* g2a,
                         const float* g2b, int m, Run run) {
    const int rc = dt_taps2_check(what, g0a, g0b, g1a, g1b, g2a, g2b, m);
    if (rc) return rc;
    DtTapsIR t = {};
    dtcwt_ifilt_taps(g0b, g0a, m, 0, t.lo, t.dlo);
    dtcwt_ifilt_taps(g1b, g1a, m, 1, t.hi, t.dhi);
    if (!g2a) return run(std::false_type{}, static_cast<const DtTapsI&>(t));
    dtcwt_ifilt_taps(g2b, g2a, m, 1, t.ba, t.dba);
    return run(std::true_type{}, t);
}

}  // namespace faoctasr
