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
// Three-filter (rotationally symmetric) banks, the entry points' optional third filter: the diagonal band hh has a bandpass filter
// h2 of its own on both axes (transform_funcs.py fwd_j1_rot, fwd_j2plus_rot, inv_j1_rot, inv_j2plus_rot); every kernel has a
// compile-time form BP for them, which a non-NULL third filter selects.
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
// The staging and the two filter passes are the four tile bodies of dtcwt_dev.h (dt_fwd1_*, dt_fwd2_*, dt_inv1, dt_inv2), which the
// scattering layers (scat.hip) and the magnitude loss (dtcwt_loss.hip) run as well; a kernel here decodes its block, declares the
// LDS arrays, calls the body and, in the forwards, applies q2c and stores.
//
// The bandpass tensor is addressed through element strides of its (n, c, orientation, row, column, re/im) axes, so any
// o_dim / ri_dim layout and any view runs without a copy; where re/im are adjacent and 8-byte aligned the pair moves as one
// float2.  The lowpass input takes (n, c, row) strides, columns unit-stride.  Outputs the kernels own (ll, y) are contiguous.
#include "dtcwt_dev.h"

namespace faoctasr {

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 forward: x [H, W] even -> ll [H, W] (optional), six complex bands [H/2, W/2] (HIGHS)
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
    const DtTile b = dt_tile(tiles_h, tiles_w);
    const long n = b.plane / C, c = b.plane % C;
    const int oi0 = b.th * J1_TH, oj0 = b.tw * J1_TW;
    dt_fwd1_rows<HIGHS, BP>(x + n * xs.n + c * xs.c, xs.r, oi0, oj0, H, W, sym, L0, L1, taps, patch, mid_lo, mid_hi, mid_ba);

    const int qi = threadIdx.x >> 5, qj = threadIdx.x & 31;
    const int oi = oi0 + 2 * qi, oj = oj0 + 2 * qj;
    if (oi >= H || oj >= W) return;                                       // H, W even: a quad is inside or outside as a whole
    const DtQuad1 v = dt_fwd1_quad<HIGHS, BP>(qi, qj, L0, L1, taps, mid_lo, mid_hi, mid_ba);
    if (ll) {
        float* lp = ll + b.plane * H * (long)W + (long)oi * W + oj;
        *reinterpret_cast<float2*>(lp) = v.ll[0];
        *reinterpret_cast<float2*>(lp + W) = v.ll[1];
    }
    if (HIGHS) {
        float* q = hi + n * hs.n + c * hs.c + (long)(oi >> 1) * hs.r + (long)(oj >> 1) * hs.w;
        dt_q2c(q, hs, vec, 0, 5, v.lh[0], v.lh[1]);
        dt_q2c(q, hs, vec, 1, 4, v.hh[0], v.hh[1]);
        dt_q2c(q, hs, vec, 2, 3, v.hl[0], v.hl[1]);
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
    const DtTile b = dt_tile(tiles_h, tiles_w);
    const long n = b.plane / C, c = b.plane % C;
    const int OH = H >> 1, OW = W >> 1;
    const int i0 = b.th * (F2_TH / 2), j0 = b.tw * (F2_TW / 2);           // first quad row / column = first index of the trees
    dt_fwd2_rows<HIGHS, BP>(x + n * xs.n + c * xs.c, xs.r, i0, j0, H, W, m, taps, patch, mid_lo, mid_hi, mid_ba);

    const int tid = threadIdx.x, path = tid >> 7, qi = (tid & 127) >> 5, qj = tid & 31;
    if (!HIGHS && path) return;
    const int oi = 2 * (i0 + qi), oj = 2 * (j0 + qj);                      // top-left of the quad in ll
    if (oi >= OH || oj >= OW) return;
    const DtQuad2 v = dt_fwd2_quad<HIGHS, BP>(path, qi, qj, m, taps, mid_lo, mid_hi, mid_ba);
    if (!path && ll) {
        float* lp = ll + b.plane * OH * (long)OW + (long)oi * OW + oj;
        *reinterpret_cast<float2*>(lp) = v.l0;
        *reinterpret_cast<float2*>(lp + OW) = v.l1;
    }
    if (HIGHS) {
        float* q = hi + n * hs.n + c * hs.c + (long)(i0 + qi) * hs.r + (long)(j0 + qj) * hs.w;
        if (path) {
            dt_q2c(q, hs, vec, 2, 3, v.l0, v.l1);                         // hl
            dt_q2c(q, hs, vec, 1, 4, v.h0, v.h1);                         // hh
        } else {
            dt_q2c(q, hs, vec, 0, 5, v.h0, v.h1);                         // lh
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
    const DtTile b = dt_tile(tiles_h, tiles_w);
    const long n = b.plane / C, c = b.plane % C;
    const float* lp = ll ? ll + n * ls.n + c * ls.c : nullptr;
    const float* hp = hi ? hi + n * hs.n + c * hs.c : nullptr;
    const auto stage = [&](int sr, int sc, float* o0, float* o1, float* o2, float* o3) { dt_stage(lp, ls, hp, hs, sr, sc, o0, o1, o2, o3); };
    dt_inv1<BP>(stage, lp != nullptr, hp != nullptr, y + b.plane * H * (long)W, b.th * J1_TH, b.tw * J1_TW, H, W, sym, L0, L1, taps, cf, mid_lo,
                mid_hi, mid_ba);
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
    const DtTile b = dt_tile(tiles_h, tiles_w);
    const long n = b.plane / C, c = b.plane % C;
    const float* lp = ll ? ll + n * ls.n + c * ls.c : nullptr;
    const float* hp = hi ? hi + n * hs.n + c * hs.c : nullptr;
    const auto stage = [&](int sr, int sc, float* o0, float* o1, float* o2, float* o3) { dt_stage(lp, ls, hp, hs, sr, sc, o0, o1, o2, o3); };
    dt_inv2<BP>(stage, lp != nullptr, hp != nullptr, y + b.plane * (2L * R) * (2L * Q), b.th * I2_TH, b.tw * I2_TW, R, Q, m2, taps, cf, mid_lo,
                mid_hi, mid_ba, tl, td);
}

}  // namespace faoctasr

using namespace faoctasr;

// The launches: run_* takes the taps of its form (BP: with the third filter) checked and packed.
template <bool BP>
static int run_fwd_j1(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                      long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W, int L0, int L1,
                      const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    if (!x || (!ll && !hi)) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    int rc, tiles_h, tiles_w;
    long blocks;
    if ((rc = dt_tiles1(what, H, W, &tiles_h, &tiles_w))) return rc;
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const DtStr hs{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si};
    if constexpr (BP) {
        if (!hi) return fail(FAOCTASR_EINVAL, "%s: the lowpass alone takes no third filter, pass a NULL third filter", what);
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
    int rc, tiles_h, tiles_w;
    long blocks;
    if ((rc = dt_tiles2f(what, H, W, &tiles_h, &tiles_w))) return rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const DtStr hs{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si};
    if constexpr (BP) {
        if (!hi) return fail(FAOCTASR_EINVAL, "%s: the lowpass alone takes no third filter, pass a NULL third filter", what);
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
    int rc, tiles_h, tiles_w;
    long blocks;
    if ((rc = dt_tiles1(what, H, W, &tiles_h, &tiles_w))) return rc;
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
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
    int rc, tiles_h, tiles_w;
    long blocks;
    if ((rc = dt_tiles2i(what, H, W, &tiles_h, &tiles_w))) return rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(dtcwt_inv_j2<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ll, DtLow{ll_sn, ll_sc, ll_sr}, hi,
                       DtStr{hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si}, y, C, H / 2, W / 2, tiles_h, tiles_w, m / 2, t);
    return check_launch(what);
}

// The entry points: the tap arguments, checked and packed by dt_with_taps*, pick the form of the launch.
extern "C" int faoctasr_dtcwt_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                     const float* h0, int L0, const float* h1, int L1, const float* h2, int L2, int mode,
                                     faoctasr_stream_t stream) {
    const char* what = "dtcwt_fwd_j1";
    return dt_with_taps1(what, h0, L0, h1, L1, h2, L2, [&](auto bp, const auto& t) {
        return run_fwd_j1<decltype(bp)::value>(what, x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, L0,
                                               L1, t, mode, stream);
    });
}

extern "C" int faoctasr_dtcwt_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* ll, float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, int hi_vec2, long N, int C, int H, int W,
                                     const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                                     const float* h2b, int m, faoctasr_stream_t stream) {
    const char* what = "dtcwt_fwd_j2";
    return dt_with_taps2(what, h0a, h0b, h1a, h1b, h2a, h2b, m, [&](auto bp, const auto& t) {
        return run_fwd_j2<decltype(bp)::value>(what, x, x_sn, x_sc, x_sr, ll, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, hi_vec2, N, C, H, W, m,
                                               t, stream);
    });
}

extern "C" int faoctasr_dtcwt_inv_j1(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                     const float* g0, int L0, const float* g1, int L1, const float* g2, int L2, int mode,
                                     faoctasr_stream_t stream) {
    const char* what = "dtcwt_inv_j1";
    return dt_with_taps1(what, g0, L0, g1, L1, g2, L2, [&](auto bp, const auto& t) {
        return run_inv_j1<decltype(bp)::value>(what, ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, L0, L1, t,
                                               mode, stream);
    });
}

extern "C" int faoctasr_dtcwt_inv_j2(const float* ll, long ll_sn, long ll_sc, long ll_sr, const float* hi, long hi_sn, long hi_sc,
                                     long hi_so, long hi_sr, long hi_sw, long hi_si, float* y, long N, int C, int H, int W,
                                     const float* g0a, const float* g0b, const float* g1a, const float* g1b, const float* g2a,
                                     const float* g2b, int m, faoctasr_stream_t stream) {
    const char* what = "dtcwt_inv_j2";
    return dt_with_tapsi(what, g0a, g0b, g1a, g1b, g2a, g2b, m, [&](auto bp, const auto& t) {
        return run_inv_j2<decltype(bp)::value>(what, ll, ll_sn, ll_sc, ll_sr, hi, hi_sn, hi_sc, hi_so, hi_sr, hi_sw, hi_si, y, N, C, H, W, m, t,
                                               stream);
    });
}
