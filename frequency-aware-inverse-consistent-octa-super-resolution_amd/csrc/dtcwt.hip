// Dual-tree complex wavelet transform, one level per launch, fp32 (pytorch_wavelets dtcwt/transform_funcs.py fwd_j1, fwd_j2plus,
// inv_j1, inv_j2plus; dtcwt/lowlevel.py colfilter .. rowifilt, q2c, c2q).  Four kernels serve the forward, the inverse and all four
// backward passes (each backward is another of the four on swapped taps, transform_funcs.py:343-488).
//
// Notation.  fold(j, N) is the half-sample symmetric extension of period 2N (MODE_SYMMETRIC of dwt.hip), applied any number of
// times; xs is x read through it, or -- level 1 in any mode but 'symmetric' -- x with zeros outside [0, N).  Filters arrive as the
// modules register them (taps reversed), so every sum below is a plain correlation with the buffer `buf`.
//
// Level 1, per axis (W first, then H), L odd:           out[i] = sum_t buf[t] xs[i + t - L/2]            ("same" size)
//   ll = lo.lo, lh = (W lo, H hi), hl = (W hi, H lo), hh = hi.hi at full resolution; the lowpass filter h0 and the highpass h1
//   may differ in length.
// Level >= 2, per axis of length r (r % 4 == 0), m even taps, always symmetric:
//   lowpass call   out[2i] = sum_t h0b[t] xs[4i + 2t + 2 - m],   out[2i+1] = sum_t h0a[t] xs[4i + 2t + 3 - m]
//   highpass call  out[2i] = sum_t h1a[t] xs[4i + 2t + 3 - m],   out[2i+1] = sum_t h1b[t] xs[4i + 2t + 2 - m]
// q2c on every 2x2 quad a=(2i,2j) b=(2i,2j+1) c=(2i+1,2j) d=(2i+1,2j+1), scaled by 1/sqrt 2 first:
//   z1 = (a - d) + i (b + c),  z2 = (a + d) + i (b - c);   orientations 15,45,75,105,135,165 = lh.z1, hh.z1, hl.z1, hl.z2, hh.z2, lh.z2.
// c2q is its inverse map: (2i,2j) = w1r + w2r, (2i,2j+1) = w1i + w2i, (2i+1,2j) = w1i - w2i, (2i+1,2j+1) = w2r - w1r, times 1/sqrt 2.
// Inverse level 1:   y = row(col(hh, g1) + col(hl, g0), g1) + row(col(lh, g1) + col(ll, g0), g0)     (H first, then W).
// Inverse level >= 2: the same sums with the 2x interpolation     out[4i + q] = sum_{t < m/2} half_q[t] xs[2 (i + t) + d_q - m/2],
//   q = 0..3, where half_q is the even or odd polyphase half of one of the two trees' filters and d_q an offset in 0..3; both
//   depend on the parity of m/2 and on whether the call is a lowpass or a highpass one (lowlevel.py:154-239; the host builds
//   the table, dtcwt_ifilt_taps below).
//
// Three-filter ("_bp", rotationally symmetric) banks: the diagonal band hh has a bandpass filter h2 of its own on both axes
// (transform_funcs.py fwd_j1_rot, fwd_j2plus_rot, inv_j1_rot, inv_j2plus_rot); every kernel has a compile-time form BP for them.
//   forward:  ba = row(x, h2),  hh = col(ba, h2);  ll, lh, hl as above.  Level 1: h2 has an odd length of its own (the halo is the
//     largest half-length of the three).  Level >= 2: (h2b, h2a) is a highpass call, with the index formula of (h1b, h1a).
//   inverse:  lo = col(lh, g1) + col(ll, g0),  hi = col(hl, g0),  ba = col(hh, g2);   y = (row(hi, g1) + row(lo, g0)) + row(ba, g2),
//     the three row sums added in this order.  Level >= 2: (g2b, g2a) is a highpass call with a third table of dtcwt_ifilt_taps.
//   The two-filter forms (BP = false) take the argument structs and compile to the instructions they had before BP existed.
//
// Every kernel: a block owns a tile of one (n, c) plane, stages its input patch (tile + halo) in LDS through the index map --
// the inverses apply c2q while staging --, runs the first pass into LDS and the second into registers, applies q2c there and
// stores.  The input is read once (plus the halo), every output written once, nothing intermediate leaves the CU; the taps
// travel by value in the kernel arguments (no device allocation, no state, capturable).  Every output is a fixed-order sum
// (t = 0 .. L-1 per pass, no atomics), whatever the tile it falls in: bit-reproducible.
//
// The bandpass tensor is addressed through element strides of its (n, c, orientation, row, column, re/im) axes, so any
// o_dim / ri_dim layout and any view runs without a copy; where re/im are adjacent and 8-byte aligned the pair moves as one
// float2.  The lowpass input takes (n, c, row) strides, columns unit-stride.  Outputs the kernels own (ll, y) are contiguous.
#include "dtcwt_dev.h"

namespace faoctasr {

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 forward
// ---------------------------------------------------------------------------------------------------------------------------
template <bool HIGHS, bool BP>
__global__ __launch_bounds__(256) void dtcwt_fwd_j1(const float* __restrict__ x, DtLow xs, float* __restrict__ ll, float* __restrict__ hi,
                                                    DtStr hs, int vec, int C, int H, int W, int tiles_h, int tiles_w, int L0, int L1,
                                                    int sym, typename DtBank<BP>::T1 taps) {
    static_assert(HIGHS || !BP, "the lowpass-only form has no third filter");
    __shared__ float patch[J1_PR][J1_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[HIGHS ? J1_PR : 1][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? J1_PR : 1][J1_TW];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tw = b % tiles_w; b /= tiles_w;
    const int th = b % tiles_h;
    const long plane = b / tiles_h;
    const long n = plane / C, c = plane % C;
    const int oi0 = th * J1_TH, oj0 = tw * J1_TW;
    const int hm = dt_halo1<BP>(L0, L1, taps), a0 = hm - (L0 >> 1), a1 = hm - (L1 >> 1);
    const int rows = J1_TH + 2 * hm, cols = J1_TW + 2 * hm;               // <= J1_PR, J1_PC
    const float* xp = x + n * xs.n + c * xs.c;

    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(oi0 - hm + r, H, sym);
        for (int cc = tid & 63; cc < cols; cc += 64) {
            const int sc = dt_map(oj0 - hm + cc, W, sym);
            patch[r][cc] = (sr >= 0 && sc >= 0) ? xp[sr * xs.r + sc] : 0.f;
        }
    }
    __syncthreads();

    {   // W pass: thread (r, cc) filters patch row r at tile column cc
        const int cc = tid & 63;
        for (int r = tid >> 6; r < rows; r += 4) {
            float lo = 0.f;
            for (int t = 0; t < L0; ++t) lo = fmaf(taps.f0[t], patch[r][cc + t + a0], lo);
            mid_lo[r][cc] = lo;
            if (HIGHS) {
                float hv = 0.f;
                for (int t = 0; t < L1; ++t) hv = fmaf(taps.f1[t], patch[r][cc + t + a1], hv);
                mid_hi[r][cc] = hv;
            }
            if constexpr (BP) {
                const int a2 = hm - (taps.L2 >> 1);
                float bv = 0.f;
                for (int t = 0; t < taps.L2; ++t) bv = fmaf(taps.f2[t], patch[r][cc + t + a2], bv);
                mid_ba[r][cc] = bv;
            }
        }
    }
    __syncthreads();

    // H pass: a thread owns one 2x2 quad of the tile (8 x 32 quads), reads the column pair as float2
    const int qi = tid >> 5, qj = tid & 31;
    const int oi = oi0 + 2 * qi, oj = oj0 + 2 * qj;
    if (oi >= H || oj >= W) return;                                       // H, W even: a quad is inside or outside as a whole
    float2 vll[2], vlh[2], vhl[2], vhh[2];
    for (int d = 0; d < 2; ++d) {
        float2 s = make_float2(0.f, 0.f);
        for (int t = 0; t < L0; ++t) {
            const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + a0][2 * qj]);
            s.x = fmaf(taps.f0[t], v.x, s.x); s.y = fmaf(taps.f0[t], v.y, s.y);
        }
        vll[d] = s;
        if (HIGHS) {
            float2 u = make_float2(0.f, 0.f), p = u, q = u;
            for (int t = 0; t < L1; ++t) {
                const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + a1][2 * qj]);
                float2 w;
                if constexpr (!BP) w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + a1][2 * qj]);
                u.x = fmaf(taps.f1[t], v.x, u.x); u.y = fmaf(taps.f1[t], v.y, u.y);
                if constexpr (!BP) { q.x = fmaf(taps.f1[t], w.x, q.x); q.y = fmaf(taps.f1[t], w.y, q.y); }
            }
            for (int t = 0; t < L0; ++t) {
                const float2 w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + a0][2 * qj]);
                p.x = fmaf(taps.f0[t], w.x, p.x); p.y = fmaf(taps.f0[t], w.y, p.y);
            }
            if constexpr (BP) {                                           // hh = col(ba, h2)
                const int a2 = hm - (taps.L2 >> 1);
                for (int t = 0; t < taps.L2; ++t) {
                    const float2 w = *reinterpret_cast<const float2*>(&mid_ba[2 * qi + d + t + a2][2 * qj]);
                    q.x = fmaf(taps.f2[t], w.x, q.x); q.y = fmaf(taps.f2[t], w.y, q.y);
                }
            }
            vlh[d] = u; vhl[d] = p; vhh[d] = q;
        }
    }
    if (ll) {
        float* lp = ll + plane * H * (long)W + (long)oi * W + oj;
        *reinterpret_cast<float2*>(lp) = vll[0];
        *reinterpret_cast<float2*>(lp + W) = vll[1];
    }
    if (HIGHS) {
        float* q = hi + n * hs.n + c * hs.c + (long)(oi >> 1) * hs.r + (long)(oj >> 1) * hs.w;
        dt_q2c(q, hs, vec, 0, 5, vlh[0], vlh[1]);
        dt_q2c(q, hs, vec, 1, 4, vhh[0], vhh[1]);
        dt_q2c(q, hs, vec, 2, 3, vhl[0], vhl[1]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level >= 2 forward: x [H, W] (multiples of 4) -> ll [H/2, W/2], six complex bands [H/4, W/4]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool HIGHS, bool BP>
__global__ __launch_bounds__(256) void dtcwt_fwd_j2(const float* __restrict__ x, DtLow xs, float* __restrict__ ll, float* __restrict__ hi,
                                                    DtStr hs, int vec, int C, int H, int W, int tiles_h, int tiles_w, int m,
                                                    typename DtBank<BP>::T2 taps) {
    static_assert(HIGHS || !BP, "the lowpass-only form has no third filter");
    __shared__ __attribute__((aligned(16))) float patch[F2_PR][F2_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[HIGHS ? F2_PR : 1][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? F2_PR : 1][F2_TW];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tw = b % tiles_w; b /= tiles_w;
    const int th = b % tiles_h;
    const long plane = b / tiles_h;
    const long n = plane / C, c = plane % C;
    const int OH = H >> 1, OW = W >> 1;
    const int i0 = th * (F2_TH / 2), j0 = tw * (F2_TW / 2);               // first quad row / column = first index of the trees
    const int rows = 2 * F2_TH + 2 * m - 4, cols = 2 * F2_TW + 2 * m - 4;  // <= F2_PR, F2_PC; patch (r, cc) is x position 4 i0 + 2 - m + r
    const float* xp = x + n * xs.n + c * xs.c;

    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(4 * i0 + 2 - m + r, H, 1);
        for (int cc = tid & 63; cc < cols; cc += 64)
            patch[r][cc] = xp[sr * xs.r + dt_map(4 * j0 + 2 - m + cc, W, 1)];
    }
    __syncthreads();

    {   // W pass: tile column cc = 2 i + p; the float2 at patch column 4 i + 2 t holds the samples at offsets 2 - m and 3 - m
        const int cc = tid & 63, i = cc >> 1, p = cc & 1;
        for (int r = tid >> 6; r < rows; r += 4) {
            float lo = 0.f, hv = 0.f, bv = 0.f;
            for (int t = 0; t < m; ++t) {
                const float2 v = *reinterpret_cast<const float2*>(&patch[r][4 * i + 2 * t]);
                lo = fmaf(p ? taps.lo1[t] : taps.lo0[t], p ? v.y : v.x, lo);
                if (HIGHS) hv = fmaf(p ? taps.hi1[t] : taps.hi0[t], p ? v.x : v.y, hv);
                if constexpr (BP) bv = fmaf(p ? taps.ba1[t] : taps.ba0[t], p ? v.x : v.y, bv);
            }
            mid_lo[r][cc] = lo;
            if (HIGHS) mid_hi[r][cc] = hv;
            if constexpr (BP) mid_ba[r][cc] = bv;
        }
    }
    __syncthreads();

    // H pass: 4 x 32 quads; threads 0..127 take the W-lowpass plane (ll, lh), threads 128..255 the W-highpass plane (hl, hh);
    // BP: the latter take hl from the W-highpass plane and hh from the W-bandpass one, with the bandpass taps
    const int path = tid >> 7, qi = (tid & 127) >> 5, qj = tid & 31;
    if (!HIGHS && path) return;
    const int oi = 2 * (i0 + qi), oj = 2 * (j0 + qj);                      // top-left of the quad in ll
    if (oi >= OH || oj >= OW) return;
    float2 l0 = make_float2(0.f, 0.f), l1 = l0, h0 = l0, h1 = l0;         // lowpass call rows 2qi, 2qi+1; highpass call likewise
    for (int t = 0; t < m; ++t) {
        const float* mp = path ? &mid_hi[HIGHS ? 4 * qi + 2 * t : 0][2 * qj] : &mid_lo[4 * qi + 2 * t][2 * qj];
        const float2 r0 = *reinterpret_cast<const float2*>(mp), r1 = *reinterpret_cast<const float2*>(mp + F2_TW);
        l0.x = fmaf(taps.lo0[t], r0.x, l0.x); l0.y = fmaf(taps.lo0[t], r0.y, l0.y);
        l1.x = fmaf(taps.lo1[t], r1.x, l1.x); l1.y = fmaf(taps.lo1[t], r1.y, l1.y);
        if constexpr (BP) {
            const float* bp = path ? &mid_ba[4 * qi + 2 * t][2 * qj] : mp;
            const float2 b0 = *reinterpret_cast<const float2*>(bp), b1 = *reinterpret_cast<const float2*>(bp + F2_TW);
            const float k0 = path ? taps.ba0[t] : taps.hi0[t], k1 = path ? taps.ba1[t] : taps.hi1[t];
            h0.x = fmaf(k0, b1.x, h0.x); h0.y = fmaf(k0, b1.y, h0.y);
            h1.x = fmaf(k1, b0.x, h1.x); h1.y = fmaf(k1, b0.y, h1.y);
        } else if (HIGHS) {
            h0.x = fmaf(taps.hi0[t], r1.x, h0.x); h0.y = fmaf(taps.hi0[t], r1.y, h0.y);
            h1.x = fmaf(taps.hi1[t], r0.x, h1.x); h1.y = fmaf(taps.hi1[t], r0.y, h1.y);
        }
    }
    if (!path && ll) {
        float* lp = ll + plane * OH * (long)OW + (long)oi * OW + oj;
        *reinterpret_cast<float2*>(lp) = l0;
        *reinterpret_cast<float2*>(lp + OW) = l1;
    }
    if (HIGHS) {
        float* q = hi + n * hs.n + c * hs.c + (long)(i0 + qi) * hs.r + (long)(j0 + qj) * hs.w;
        if (path) {
            dt_q2c(q, hs, vec, 2, 3, l0, l1);                             // hl
            dt_q2c(q, hs, vec, 1, 4, h0, h1);                             // hh
        } else {
            dt_q2c(q, hs, vec, 0, 5, h0, h1);                             // lh
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 inverse: ll [H, W], six complex bands [H/2, W/2] (either may be null = zeros, its path is skipped) -> y [H, W]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void dtcwt_inv_j1(const float* __restrict__ ll, DtLow ls, const float* __restrict__ hi, DtStr hs,
                                                    float* __restrict__ y, int C, int H, int W, int tiles_h, int tiles_w, int L0, int L1,
                                                    int sym, typename DtBank<BP>::T1 taps) {
    __shared__ float cf[4][J1_PR][J1_PC];
    __shared__ float mid_lo[J1_TH][J1_PC], mid_hi[J1_TH][J1_PC], mid_ba[BP ? J1_TH : 1][J1_PC];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tw = b % tiles_w; b /= tiles_w;
    const int th = b % tiles_h;
    const long plane = b / tiles_h;
    const long n = plane / C, c = plane % C;
    const int t0 = th * J1_TH, s0 = tw * J1_TW;
    const int hm = dt_halo1<BP>(L0, L1, taps), a0 = hm - (L0 >> 1), a1 = hm - (L1 >> 1);
    const int rows = J1_TH + 2 * hm, cols = J1_TW + 2 * hm;
    const float* lp = ll ? ll + n * ls.n + c * ls.c : nullptr;
    const float* hp = hi ? hi + n * hs.n + c * hs.c : nullptr;

    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(t0 - hm + r, H, sym);
        for (int cc = tid & 63; cc < cols; cc += 64) {
            const int sc = dt_map(s0 - hm + cc, W, sym);
            if (sr >= 0 && sc >= 0) dt_stage(lp, ls, hp, hs, sr, sc, &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
            else cf[0][r][cc] = cf[1][r][cc] = cf[2][r][cc] = cf[3][r][cc] = 0.f;
        }
    }
    __syncthreads();

    // H pass: lo = col(lh, g1) + col(ll, g0), hi = col(hh, g1) + col(hl, g0), for every tile row and patch column;
    // BP: hi = col(hl, g0), ba = col(hh, g2)
    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {
        for (int cc = tid & 63; cc < cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            if (hp) {
                for (int t = 0; t < L1; ++t) {
                    l1 = fmaf(taps.f1[t], cf[1][tt + t + a1][cc], l1);
                    if constexpr (!BP) h1 = fmaf(taps.f1[t], cf[3][tt + t + a1][cc], h1);
                }
                for (int t = 0; t < L0; ++t) h0 = fmaf(taps.f0[t], cf[2][tt + t + a0][cc], h0);
                if constexpr (BP) {
                    const int a2 = hm - (taps.L2 >> 1);
                    for (int t = 0; t < taps.L2; ++t) h1 = fmaf(taps.f2[t], cf[3][tt + t + a2][cc], h1);
                }
            }
            if (lp)
                for (int t = 0; t < L0; ++t) l0 = fmaf(taps.f0[t], cf[0][tt + t + a0][cc], l0);
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) { mid_hi[tt][cc] = h0; mid_ba[tt][cc] = h1; }
            else mid_hi[tt][cc] = h1 + h0;
        }
    }
    __syncthreads();

    float* yp = y + plane * H * (long)W;
    const int ss = tid & 63, s = s0 + ss;
    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= H || s >= W) continue;
        float vh = 0.f, vl = 0.f;
        if (hp)
            for (int k = 0; k < L1; ++k) vh = fmaf(taps.f1[k], mid_hi[tt][ss + k + a1], vh);
        for (int k = 0; k < L0; ++k) vl = fmaf(taps.f0[k], mid_lo[tt][ss + k + a0], vl);
        if constexpr (BP) {
            const int a2 = hm - (taps.L2 >> 1);
            float vb = 0.f;
            if (hp)
                for (int k = 0; k < taps.L2; ++k) vb = fmaf(taps.f2[k], mid_ba[tt][ss + k + a2], vb);
            yp[(long)t * W + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * W + s] = vh + vl;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level >= 2 inverse: ll [R, Q], six complex bands [R/2, Q/2] (either may be null) -> y [2R, 2Q]; always symmetric
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void dtcwt_inv_j2(const float* __restrict__ ll, DtLow ls, const float* __restrict__ hi, DtStr hs,
                                                    float* __restrict__ y, int C, int R, int Q, int tiles_h, int tiles_w, int m2,
                                                    typename DtBank<BP>::TI taps) {
    __shared__ float cf[4][I2_PR][I2_PC];
    __shared__ float mid_lo[I2_TH][I2_PC], mid_hi[I2_TH][I2_PC], mid_ba[BP ? I2_TH : 1][I2_PC];
    __shared__ float tl[BP ? 3 : 2][4][DT_MAXL / 2];
    __shared__ int td[BP ? 3 : 2][4];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tw = b % tiles_w; b /= tiles_w;
    const int th = b % tiles_h;
    const long plane = b / tiles_h;
    const long n = plane / C, c = plane % C;
    const int t0 = th * I2_TH, s0 = tw * I2_TW, OH = 2 * R, OW = 2 * Q;
    const int i0 = t0 >> 2, j0 = s0 >> 2;
    const int rows = I2_TH / 2 + 2 * m2, cols = I2_TW / 2 + 2 * m2;      // patch (r, cc) is coefficient position 2 i0 - m2 + r
    const float* lp = ll ? ll + n * ls.n + c * ls.c : nullptr;
    const float* hp = hi ? hi + n * hs.n + c * hs.c : nullptr;

    if (tid < 4 * (DT_MAXL / 2)) {                                        // the per-phase taps, for the lane-varying phase of the W pass
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
            dt_stage(lp, ls, hp, hs, sr, dt_map(2 * j0 - m2 + cc, Q, 1), &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
    }
    __syncthreads();

    // H pass: a wave takes a tile row (its phase q is uniform), lanes the patch columns
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int q = tt & 3, ii = tt >> 2;                               // t0 is a multiple of 4
        const int rl = 2 * ii + td[0][q], rh = 2 * ii + td[1][q], rb = 2 * ii + td[BP ? 2 : 1][q];
        for (int cc = tid & 63; cc < cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            if (hp)
                for (int t = 0; t < m2; ++t) {
                    l1 = fmaf(tl[1][q][t], cf[1][rh + 2 * t][cc], l1);
                    h1 = fmaf(tl[BP ? 2 : 1][q][t], cf[3][rb + 2 * t][cc], h1);     // BP: ba = col(hh, g2)
                    h0 = fmaf(tl[0][q][t], cf[2][rl + 2 * t][cc], h0);
                }
            if (lp)
                for (int t = 0; t < m2; ++t) l0 = fmaf(tl[0][q][t], cf[0][rl + 2 * t][cc], l0);
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) { mid_hi[tt][cc] = h0; mid_ba[tt][cc] = h1; }
            else mid_hi[tt][cc] = h1 + h0;
        }
    }
    __syncthreads();

    float* yp = y + plane * OH * (long)OW;
    const int ss = tid & 63, s = s0 + ss, q = ss & 3, jj = ss >> 2;
    const int cl = 2 * jj + td[0][q], ch = 2 * jj + td[1][q];
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= OH || s >= OW) continue;
        float vh = 0.f, vl = 0.f;
        if (hp)
            for (int k = 0; k < m2; ++k) vh = fmaf(tl[1][q][k], mid_hi[tt][ch + 2 * k], vh);
        for (int k = 0; k < m2; ++k) vl = fmaf(tl[0][q][k], mid_lo[tt][cl + 2 * k], vl);
        if constexpr (BP) {
            const int cb = 2 * jj + td[2][q];
            float vb = 0.f;
            if (hp)
                for (int k = 0; k < m2; ++k) vb = fmaf(tl[2][q][k], mid_ba[tt][cb + 2 * k], vb);
            yp[(long)t * OW + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * OW + s] = vh + vl;
        }
    }
}

}  // namespace faoctasr

using namespace faoctasr;

// The entry points of a kernel's two forms share everything but the taps: run_* takes them checked and packed.
template <bool BP>
static int run_fwd_j1(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                      long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W, int L0, int L1,
                      const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    if (!x || (!ll && !hi)) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be even and at least 2", what, H, W);
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    const int tiles_h = (H + J1_TH - 1) / J1_TH, tiles_w = (W + J1_TW - 1) / J1_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const DtStr hs{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si};
    if constexpr (BP) {
        if (!hi) return fail(FAOCTASR_EINVAL, "%s: the lowpass alone takes no third filter, call dtcwt_fwd_j1", what);
        hipLaunchKernelGGL((dtcwt_fwd_j1<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, hi_vec2, C,
                           H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    } else if (hi) {
        hipLaunchKernelGGL((dtcwt_fwd_j1<true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, hi_vec2, C,
                           H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    } else {
        hipLaunchKernelGGL((dtcwt_fwd_j1<false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, 0, C, H, W,
                           tiles_h, tiles_w, L0, L1, mode == 1, t);
    }
    return check_launch(what);
}

template <bool BP>
static int run_fwd_j2(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                      long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W, int m,
                      const typename DtBank<BP>::T2& t, faoctasr_stream_t stream) {
    if (!x || (!ll && !hi)) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be multiples of 4", what, H, W);
    const int tiles_h = (H / 2 + F2_TH - 1) / F2_TH, tiles_w = (W / 2 + F2_TW - 1) / F2_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const DtStr hs{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si};
    if constexpr (BP) {
        if (!hi) return fail(FAOCTASR_EINVAL, "%s: the lowpass alone takes no third filter, call dtcwt_fwd_j2", what);
        hipLaunchKernelGGL((dtcwt_fwd_j2<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, hi_vec2, C,
                           H, W, tiles_h, tiles_w, m, t);
    } else if (hi) {
        hipLaunchKernelGGL((dtcwt_fwd_j2<true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, hi_vec2, C,
                           H, W, tiles_h, tiles_w, m, t);
    } else {
        hipLaunchKernelGGL((dtcwt_fwd_j2<false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, ll, hi, hs, 0, C, H, W,
                           tiles_h, tiles_w, m, t);
    }
    return check_launch(what);
}

template <bool BP>
static int run_inv_j1(const char* what, const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                      long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W, int L0, int L1,
                      const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    if (!y || (!ll && !hi)) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be even and at least 2", what, H, W);
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    const int tiles_h = (H + J1_TH - 1) / J1_TH, tiles_w = (W + J1_TW - 1) / J1_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(dtcwt_inv_j1<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ll, DtLow{ll_sn, ll_sc, ll_sr}, hi,
                       DtStr{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si}, y, C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    return check_launch(what);
}

template <bool BP>
static int run_inv_j2(const char* what, const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                      long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W, int m,
                      const typename DtBank<BP>::TI& t, faoctasr_stream_t stream) {
    if (!y || (!ll && !hi)) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: the result's H %d W %d must be multiples of 4", what, H, W);
    const int tiles_h = (H + I2_TH - 1) / I2_TH, tiles_w = (W + I2_TW - 1) / I2_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(dtcwt_inv_j2<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ll, DtLow{ll_sn, ll_sc, ll_sr}, hi,
                       DtStr{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si}, y, C, H / 2, W / 2, tiles_h, tiles_w, m / 2, t);
    return check_launch(what);
}

extern "C" int faoctasr_dtcwt_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                     const float* h0, int L0, const float* h1, int L1, int mode, faoctasr_stream_t stream) {
    DtTaps1 t;
    const int rc = dt_taps1("dtcwt_fwd_j1", h0, L0, h1, L1, &t);
    if (rc) return rc;
    return run_fwd_j1<false>("dtcwt_fwd_j1", x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, L0, L1, t,
                             mode, stream);
}

extern "C" int faoctasr_dtcwt_fwd_j1_bp(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                        long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                        const float* h0, int L0, const float* h1, int L1, const float* h2, int L2, int mode,
                                        faoctasr_stream_t stream) {
    DtTaps1R t;
    const int rc = dt_taps1r("dtcwt_fwd_j1_bp", h0, L0, h1, L1, h2, L2, &t);
    if (rc) return rc;
    return run_fwd_j1<true>("dtcwt_fwd_j1_bp", x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, L0, L1,
                            t, mode, stream);
}

extern "C" int faoctasr_dtcwt_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                     const float* h0a, const float* h0b, const float* h1a, const float* h1b, int m,
                                     faoctasr_stream_t stream) {
    const int rc = dt_taps2_check("dtcwt_fwd_j2", h0a, h0b, h1a, h1b, m);
    if (rc) return rc;
    DtTaps2 t = {};
    dt_taps2_fill(&t, h0a, h0b, h1a, h1b, m);
    return run_fwd_j2<false>("dtcwt_fwd_j2", x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, m, t,
                             stream);
}

extern "C" int faoctasr_dtcwt_fwd_j2_bp(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                        long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                        const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                                        const float* h2b, int m, faoctasr_stream_t stream) {
    const int rc = dt_taps2r_check("dtcwt_fwd_j2_bp", h0a, h0b, h1a, h1b, h2a, h2b, m);
    if (rc) return rc;
    DtTaps2R t = {};
    dt_taps2_fill(&t, h0a, h0b, h1a, h1b, h2a, h2b, m);
    return run_fwd_j2<true>("dtcwt_fwd_j2_bp", x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, m, t,
                            stream);
}

extern "C" int faoctasr_dtcwt_inv_j1(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                     const float* g0, int L0, const float* g1, int L1, int mode, faoctasr_stream_t stream) {
    DtTaps1 t;
    const int rc = dt_taps1("dtcwt_inv_j1", g0, L0, g1, L1, &t);
    if (rc) return rc;
    return run_inv_j1<false>("dtcwt_inv_j1", ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, L0, L1, t, mode,
                             stream);
}

extern "C" int faoctasr_dtcwt_inv_j1_bp(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                        long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                        const float* g0, int L0, const float* g1, int L1, const float* g2, int L2, int mode,
                                        faoctasr_stream_t stream) {
    DtTaps1R t;
    const int rc = dt_taps1r("dtcwt_inv_j1_bp", g0, L0, g1, L1, g2, L2, &t);
    if (rc) return rc;
    return run_inv_j1<true>("dtcwt_inv_j1_bp", ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, L0, L1, t,
                            mode, stream);
}

extern "C" int faoctasr_dtcwt_inv_j2(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                     const float* g0a, const float* g0b, const float* g1a, const float* g1b, int m,
                                     faoctasr_stream_t stream) {
    const int rc = dt_taps2_check("dtcwt_inv_j2", g0a, g0b, g1a, g1b, m);
    if (rc) return rc;
    DtTapsI t = {};
    dtcwt_ifilt_taps(g0b, g0a, m, 0, t.lo, t.dlo);                        // colifilt(X, g0b, g0a, False)
    dtcwt_ifilt_taps(g1b, g1a, m, 1, t.hi, t.dhi);                        // colifilt(X, g1b, g1a, True)
    return run_inv_j2<false>("dtcwt_inv_j2", ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, m, t, stream);
}

extern "C" int faoctasr_dtcwt_inv_j2_bp(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                        long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                        const float* g0a, const float* g0b, const float* g1a, const float* g1b, const float* g2a,
                                        const float* g2b, int m, faoctasr_stream_t stream) {
    const int rc = dt_taps2r_check("dtcwt_inv_j2_bp", g0a, g0b, g1a, g1b, g2a, g2b, m);
    if (rc) return rc;
    DtTapsIR t = {};
    dtcwt_ifilt_taps(g0b, g0a, m, 0, t.lo, t.dlo);                        // colifilt(X, g0b, g0a, False)
    dtcwt_ifilt_taps(g1b, g1a, m, 1, t.hi, t.dhi);                        // colifilt(X, g1b, g1a, True)
    dtcwt_ifilt_taps(g2b, g2a, m, 1, t.ba, t.dba);                        // colifilt(X, g2b, g2a, True)
    return run_inv_j2<true>("dtcwt_inv_j2_bp", ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, m, t, stream);
}
