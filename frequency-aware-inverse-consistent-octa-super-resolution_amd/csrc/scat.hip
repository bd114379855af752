// DTCWT scattering layers, fp32 (pytorch_wavelets scatternet/lowlevel.py ScatLayerj1_f, ScatLayerj2_f): a dual-tree level, the
// smoothed complex magnitude of its six orientations and the 2x2 average of its lowpass, in one launch; the backward likewise.
//
// The four kernels run the four tile bodies of dtcwt_dev.h that dtcwt.hip runs -- tiles, LDS staging, index maps and filter sums
// are written once, there -- and hold only the pointwise part of the layer, in the place of the transform's bandpass stores and loads:
//
// forward, in the registers that hold a quad's ll, lh, hl, hh after the second pass:
//   z_o = q2c of the quad (six complex values),  r_o = sqrt(re^2 + im^2 + b^2),  mag_o = r_o - b,  phase_o = (re / r_o, im / r_o)
//   low = mean of the quad's four ll values (pool) or ll itself at full resolution (level 1 only: the first stage of ScatLayerj2)
//   colour form (C == 3): r_o = sqrt(sum_c (re_c^2 + im_c^2) + b^2), one magnitude per orientation, phase_{o,c} = z_{o,c} / r_o; the
//   block runs its tile's three channels one after the other and keeps their 3 x 12 band values in registers.
//   phase == NULL: nothing is saved (a forward that no backward follows).
// backward, while staging a coefficient position (sr, sc) of the inverse:
//   ll = 0.25 dlow[sr / 2][sc / 2] (pool: the adjoint of the mean) or dlow[sr][sc];   z_o = dmag_o[sr / 2][sc / 2] phase_o[sr / 2][sc / 2],
//   c2q applied to the pairs; the two filter passes are the inverse's, on the analysis taps (level 1) or on them with trees a and
//   b swapped (level 2) -- the exact adjoint.  The colour form is a zero channel stride of dmag.
//
// Three-filter banks (an entry point's optional third filter), ScatLayerj1_rot_f / ScatLayerj2_rot_f: every kernel passes its
// compile-time form BP on to the tile body --
// forward  ba = row(x, h2), hh = col(ba, h2);  backward  hi = col(hl, h0), ba = col(hh, h2), dx = (row(hi, h1) + row(lo, h0)) + row(ba, h2)
// -- and the pointwise part is the same for both.  The forwards loop over their channels around the body's barriers, so every thread
// stays in the loop (`live` guards the quad); the backwards hand the body a stager (sc_stage) and have every input present.
//
// Addressing, in elements, rows always contiguous: low (n, c) strides, mag / dmag (n, orientation, c) strides, so a launch writes
// into (reads from) slices of the layer's output Z (its cotangent); phase is a contiguous (N, 6, C, H', W', 2) tensor, one float2
// per value.  The input x takes (n, c, row) strides; dx is contiguous.  Taps travel by value, nothing is allocated, no state,
// every sum in a fixed order: capturable and bit-reproducible.
#include "dtcwt_dev.h"

namespace faoctasr {

struct ScLow { long n, c; };
struct ScMag { long n, o, c; };

// magnitudes and phasors of one orientation over NC channels (NC == 1, or 3 reduced to one magnitude)
template <int NC>
__device__ __forceinline__ void sc_emit(const float2 (&z)[NC], float* mag, long mag_c, float2* ph, long ph_c, float b, float b2, bool colour) {
    if (colour) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) s += z[k].x * z[k].x + z[k].y * z[k].y;
        const float r = sqrtf(s + b2);
        *mag = r - b;
        if (ph) {
#pragma unroll
            for (int k = 0; k < NC; ++k) ph[k * ph_c] = make_float2(z[k].x / r, z[k].y / r);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const float r = sqrtf(z[k].x * z[k].x + z[k].y * z[k].y + b2);
            mag[k * mag_c] = r - b;
            if (ph) ph[k * ph_c] = make_float2(z[k].x / r, z[k].y / r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 forward: x [H, W] even -> low [H/2, W/2] (pool) or [H, W], mag and phase [H/2, W/2].  COLOUR: a block takes the three
// channels of its tile (the grid has N planes), else one (N * C planes)
// ---------------------------------------------------------------------------------------------------------------------------
template <bool COLOUR, bool BP>
__global__ __launch_bounds__(256) void scat_fwd_j1(const float* __restrict__ x, DtLow xs, float* __restrict__ low, ScLow ls, int pool,
                                                   float* __restrict__ mag, ScMag ms, float2* __restrict__ phase, float b, float b2, int C, int H,
                                                   int W, int tiles_h, int tiles_w, int L0, int L1, int sym, typename DtBank<BP>::T1 taps) {
    constexpr int NC = COLOUR ? 3 : 1;
    __shared__ float patch[J1_PR][J1_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? J1_PR : 1][J1_TW];
    const DtTile t = dt_tile(tiles_h, tiles_w);
    const long n = COLOUR ? t.plane : t.plane / C, c0 = COLOUR ? 0 : t.plane % C;
    const int oi0 = t.th * J1_TH, oj0 = t.tw * J1_TW;
    const int qi = threadIdx.x >> 5, qj = threadIdx.x & 31;               // H pass: a thread owns one 2x2 quad of the tile
    const int oi = oi0 + 2 * qi, oj = oj0 + 2 * qj;
    const bool live = oi < H && oj < W;                                   // H, W even: a quad is inside or outside as a whole
    const int OH = H >> 1, OW = W >> 1, pi = oi >> 1, pj = oj >> 1;
    float2 z[6][NC];

#pragma unroll
    for (int k = 0; k < NC; ++k) {                                        // every thread stays through the channels' barriers
        const long c = c0 + k;
        dt_fwd1_rows<true, BP>(x + n * xs.n + c * xs.c, xs.r, oi0, oj0, H, W, sym, L0, L1, taps, patch, mid_lo, mid_hi, mid_ba);
        if (live) {
            const DtQuad1 v = dt_fwd1_quad<true, BP>(qi, qj, L0, L1, taps, mid_lo, mid_hi, mid_ba);
            float* lp = low + n * ls.n + c * ls.c;
            if (pool) {
                lp[(long)pi * OW + pj] = 0.25f * ((v.ll[0].x + v.ll[0].y) + (v.ll[1].x + v.ll[1].y));
            } else {
                *reinterpret_cast<float2*>(lp + (long)oi * W + oj) = v.ll[0];
                *reinterpret_cast<float2*>(lp + (long)(oi + 1) * W + oj) = v.ll[1];
            }
            dt_q2c_val(v.lh[0], v.lh[1], &z[0][k], &z[5][k]);
            dt_q2c_val(v.hh[0], v.hh[1], &z[1][k], &z[4][k]);
            dt_q2c_val(v.hl[0], v.hl[1], &z[2][k], &z[3][k]);
        }
    }
    if (!live) return;
    const long hw = (long)OH * OW, at = (long)pi * OW + pj;
#pragma unroll
    for (int o = 0; o < 6; ++o)
        sc_emit<NC>(z[o], mag + n * ms.n + o * ms.o + c0 * ms.c + at, ms.c, phase ? phase + ((n * 6 + o) * C + c0) * hw + at : nullptr, hw, b, b2,
                    COLOUR);
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 2 forward: x [H, W] (multiples of 4) -> low [H/4, W/4] (the 2x2 mean of the level's lowpass), mag and phase [H/4, W/4]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool COLOUR, bool BP>
__global__ __launch_bounds__(256) void scat_fwd_j2(const float* __restrict__ x, DtLow xs, float* __restrict__ low, ScLow ls,
                                                   float* __restrict__ mag, ScMag ms, float2* __restrict__ phase, float b, float b2, int C, int H,
                                                   int W, int tiles_h, int tiles_w, int m, typename DtBank<BP>::T2 taps) {
    constexpr int NC = COLOUR ? 3 : 1;
    __shared__ __attribute__((aligned(16))) float patch[F2_PR][F2_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? F2_PR : 1][F2_TW];
    const DtTile tile = dt_tile(tiles_h, tiles_w);
    if (COLOUR) C = 3;
    const long n = COLOUR ? tile.plane : tile.plane / C, c0 = COLOUR ? 0 : tile.plane % C;
    const int OH = H >> 2, OW = W >> 2;                                    // of low, mag and phase
    const int i0 = tile.th * (F2_TH / 2), j0 = tile.tw * (F2_TW / 2);     // first quad row / column = first index of the trees
    const int tid = threadIdx.x, path = tid >> 7, qi = (tid & 127) >> 5, qj = tid & 31;
    const int pi = i0 + qi, pj = j0 + qj;
    const bool live = pi < OH && pj < OW;
    float2 za[4][NC];                                                     // path 0: lh z1, z2 (15, 165); path 1: hl z1, z2 (75, 105), hh z1, z2 (45, 135)

#pragma unroll
    for (int k = 0; k < NC; ++k) {                                        // every thread stays through the channels' barriers
        const long c = c0 + k;
        dt_fwd2_rows<true, BP>(x + n * xs.n + c * xs.c, xs.r, i0, j0, H, W, m, taps, patch, mid_lo, mid_hi, mid_ba);
        if (live) {
            const DtQuad2 v = dt_fwd2_quad<true, BP>(path, qi, qj, m, taps, mid_lo, mid_hi, mid_ba);
            if (path) {
                dt_q2c_val(v.l0, v.l1, &za[0][k], &za[1][k]);             // hl
                dt_q2c_val(v.h0, v.h1, &za[2][k], &za[3][k]);             // hh
            } else {
                low[n * ls.n + c * ls.c + (long)pi * OW + pj] = 0.25f * ((v.l0.x + v.l0.y) + (v.l1.x + v.l1.y));
                dt_q2c_val(v.h0, v.h1, &za[0][k], &za[1][k]);             // lh
                za[2][k] = za[3][k] = make_float2(0.f, 0.f);
            }
        }
    }
    if (!live) return;
    const long hw = (long)OH * OW, at = (long)pi * OW + pj;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!path && j >= 2) break;
        const int o = path ? (j == 0 ? 2 : j == 1 ? 3 : j == 2 ? 1 : 4) : (j == 0 ? 0 : 5);
        sc_emit<NC>(za[j], mag + n * ms.n + o * ms.o + c0 * ms.c + at, ms.c, phase ? phase + ((n * 6 + o) * C + c0) * hw + at : nullptr, hw, b, b2,
                    COLOUR);
    }
}

// one coefficient position (sr, sc) of the four full-resolution planes ll, lh, hl, hh from the layer's cotangents and phasors
__device__ __forceinline__ void sc_stage(const float* lp, int pool, int lw, const float* dm, long mo, const float2* ph, long po, int pw, int sr,
                                         int sc, float* o0, float* o1, float* o2, float* o3) {
    *o0 = pool ? 0.25f * lp[(long)(sr >> 1) * lw + (sc >> 1)] : lp[(long)sr * lw + sc];
    const long at = (long)(sr >> 1) * pw + (sc >> 1);
    const int pr = sr & 1, pc = sc & 1;
    const bool im = pr ^ pc;                                              // (0,1) and (1,0) take the imaginary parts
    float w[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) {
        const float2 p = ph[o * po + at];
        w[o] = dm[o * mo + at] * (im ? p.y : p.x);
    }
    *o1 = dt_c2q_val(w[0], w[5], pr, pc);                                 // lh: 15, 165
    *o2 = dt_c2q_val(w[2], w[3], pr, pc);                                 // hl: 75, 105
    *o3 = dt_c2q_val(w[1], w[4], pr, pc);                                 // hh: 45, 135
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 backward: dlow [H/2, W/2] (pool) or [H, W], dmag and phase [H/2, W/2] -> dx [H, W]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void scat_bwd_j1(const float* __restrict__ dlow, ScLow ls, int pool, const float* __restrict__ dmag, ScMag ms,
                                                   const float2* __restrict__ phase, float* __restrict__ dx, int C, int H, int W, int tiles_h,
                                                   int tiles_w, int L0, int L1, int sym, typename DtBank<BP>::T1 taps) {
    __shared__ float cf[4][J1_PR][J1_PC];
    __shared__ float mid_lo[J1_TH][J1_PC], mid_hi[J1_TH][J1_PC], mid_ba[BP ? J1_TH : 1][J1_PC];
    const DtTile t = dt_tile(tiles_h, tiles_w);
    const long n = t.plane / C, c = t.plane % C;
    const int OW = W >> 1;
    const long hw = (long)(H >> 1) * OW;
    const float* lp = dlow + n * ls.n + c * ls.c;
    const float* dm = dmag + n * ms.n + c * ms.c;
    const float2* ph = phase + (n * 6 * C + c) * hw;
    const auto stage = [&](int sr, int sc, float* o0, float* o1, float* o2, float* o3) {
        sc_stage(lp, pool, pool ? OW : W, dm, ms.o, ph, C * hw, OW, sr, sc, o0, o1, o2, o3);
    };
    dt_inv1<BP>(stage, true, true, dx + t.plane * H * (long)W, t.th * J1_TH, t.tw * J1_TW, H, W, sym, L0, L1, taps, cf, mid_lo, mid_hi, mid_ba);
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 2 backward: dlow, dmag and phase [R/2, Q/2] -> dx [2R, 2Q]; always symmetric
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void scat_bwd_j2(const float* __restrict__ dlow, ScLow ls, const float* __restrict__ dmag, ScMag ms,
                                                   const float2* __restrict__ phase, float* __restrict__ dx, int C, int R, int Q, int tiles_h,
                                                   int tiles_w, int m2, typename DtBank<BP>::TI taps) {
    __shared__ float cf[4][I2_PR][I2_PC];
    __shared__ float mid_lo[I2_TH][I2_PC], mid_hi[I2_TH][I2_PC], mid_ba[BP ? I2_TH : 1][I2_PC];
    __shared__ float tl[BP ? 3 : 2][4][DT_MAXL / 2];
    __shared__ int td[BP ? 3 : 2][4];
    const DtTile t = dt_tile(tiles_h, tiles_w);
    const long n = t.plane / C, c = t.plane % C;
    const int PW = Q >> 1;
    const long hw = (long)(R >> 1) * PW;
    const float* lp = dlow + n * ls.n + c * ls.c;
    const float* dm = dmag + n * ms.n + c * ms.c;
    const float2* ph = phase + (n * 6 * C + c) * hw;
    const auto stage = [&](int sr, int sc, float* o0, float* o1, float* o2, float* o3) {
        sc_stage(lp, 1, PW, dm, ms.o, ph, C * hw, PW, sr, sc, o0, o1, o2, o3);
    };
    dt_inv2<BP>(stage, true, true, dx + t.plane * (2 * R) * (long)(2 * Q), t.th * I2_TH, t.tw * I2_TW, R, Q, m2, taps, cf, mid_lo, mid_hi, mid_ba,
                tl, td);
}

static int sc_common(const char* what, const void* a, const void* b, const void* c, int colour, int C) {
    if (!a || !b || !c) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (colour && C != 3) return fail(FAOCTASR_EINVAL, "%s: the colour form takes 3 channels, got %d", what, C);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

// The launches: run_* takes the taps of its form (BP: with the third filter) checked and packed.
template <bool BP>
static int run_fwd_j1(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                      float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C,
                      int H, int W, int L0, int L1, const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    int rc, tiles_h, tiles_w;
    if ((rc = sc_common(what, x, low, mag, colour, C))) return rc;
    if ((rc = dt_tiles1(what, H, W, &tiles_h, &tiles_w))) return rc;
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    long blocks;
    if ((rc = dt_blocks(what, N, colour ? 1 : C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const ScLow ls{low_sn, low_sc};
    const ScMag ms{mag_sn, mag_so, mag_sc};
    if (colour)
        hipLaunchKernelGGL((scat_fwd_j1<true, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, pool != 0, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    else
        hipLaunchKernelGGL((scat_fwd_j1<false, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, pool != 0, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    return check_launch(what);
}

template <bool BP>
static int run_fwd_j2(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                      long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C, int H, int W,
                      int m, const typename DtBank<BP>::T2& t, faoctasr_stream_t stream) {
    int rc, tiles_h, tiles_w;
    if ((rc = sc_common(what, x, low, mag, colour, C))) return rc;
    if ((rc = dt_tiles2f(what, H, W, &tiles_h, &tiles_w))) return rc;
    long blocks;
    if ((rc = dt_blocks(what, N, colour ? 1 : C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const ScLow ls{low_sn, low_sc};
    const ScMag ms{mag_sn, mag_so, mag_sc};
    if (colour)
        hipLaunchKernelGGL((scat_fwd_j2<true, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, m, t);
    else
        hipLaunchKernelGGL((scat_fwd_j2<false, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, m, t);
    return check_launch(what);
}

template <bool BP>
static int run_bwd_j1(const char* what, const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                      long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, int L0, int L1,
                      const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    if (!dlow || !dmag || !phase || !dx) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    int rc, tiles_h, tiles_w;
    if ((rc = dt_tiles1(what, H, W, &tiles_h, &tiles_w))) return rc;
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    long blocks;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(scat_bwd_j1<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dlow, ScLow{dlow_sn, dlow_sc}, pool != 0, dmag,
                       ScMag{dmag_sn, dmag_so, dmag_sc}, reinterpret_cast<const float2*>(phase), dx, C, H, W, tiles_h, tiles_w, L0, L1,
                       mode == 1, t);
    return check_launch(what);
}

template <bool BP>
static int run_bwd_j2(const char* what, const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so,
                      long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, int m, const typename DtBank<BP>::TI& t,
                      faoctasr_stream_t stream) {
    if (!dlow || !dmag || !phase || !dx) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    int rc, tiles_h, tiles_w;
    if ((rc = dt_tiles2i(what, H, W, &tiles_h, &tiles_w))) return rc;
    long blocks;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(scat_bwd_j2<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dlow, ScLow{dlow_sn, dlow_sc}, dmag,
                       ScMag{dmag_sn, dmag_so, dmag_sc}, reinterpret_cast<const float2*>(phase), dx, C, H / 2, W / 2, tiles_h, tiles_w, m / 2, t);
    return check_launch(what);
}

// The entry points: the tap arguments, checked and packed by dt_with_taps*, pick the form of the launch.
extern "C" int faoctasr_scat_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                                    float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2,
                                    long N, int C, int H, int W, const float* h0, int L0, const float* h1, int L1, const float* h2, int L2,
                                    int mode, faoctasr_stream_t stream) {
    const char* what = "scat_fwd_j1";
    return dt_with_taps1(what, h0, L0, h1, L1, h2, L2, [&](auto bp, const auto& t) {
        return run_fwd_j1<decltype(bp)::value>(what, x, x_sn, x_sc, x_sr, low, low_sn, low_sc, pool, mag, mag_sn, mag_so, mag_sc, phase, colour, bias,
                                               bias2, N, C, H, W, L0, L1, t, mode, stream);
    });
}

extern "C" int faoctasr_scat_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                                    long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C,
                                    int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                                    const float* h2b, int m, faoctasr_stream_t stream) {
    const char* what = "scat_fwd_j2";
    return dt_with_taps2(what, h0a, h0b, h1a, h1b, h2a, h2b, m, [&](auto bp, const auto& t) {
        return run_fwd_j2<decltype(bp)::value>(what, x, x_sn, x_sc, x_sr, low, low_sn, low_sc, mag, mag_sn, mag_so, mag_sc, phase, colour, bias, bias2,
                                               N, C, H, W, m, t, stream);
    });
}

extern "C" int faoctasr_scat_bwd_j1(const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                                    long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, const float* h0, int L0,
                                    const float* h1, int L1, const float* h2, int L2, int mode, faoctasr_stream_t stream) {
    const char* what = "scat_bwd_j1";
    return dt_with_taps1(what, h0, L0, h1, L1, h2, L2, [&](auto bp, const auto& t) {
        return run_bwd_j1<decltype(bp)::value>(what, dlow, dlow_sn, dlow_sc, pool, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, L0, L1, t,
                                               mode, stream);
    });
}

// the inverse on the forward's analysis taps with the trees swapped: g0a = h0b, g0b = h0a, and so for the other two pairs
extern "C" int faoctasr_scat_bwd_j2(const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so, long dmag_sc,
                                    const float* phase, float* dx, long N, int C, int H, int W, const float* h0a, const float* h0b,
                                    const float* h1a, const float* h1b, const float* h2a, const float* h2b, int m, faoctasr_stream_t stream) {
    const char* what = "scat_bwd_j2";
    return dt_with_tapsi(what, h0b, h0a, h1b, h1a, h2b, h2a, m, [&](auto bp, const auto& t) {
        return run_bwd_j2<decltype(bp)::value>(what, dlow, dlow_sn, dlow_sc, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, m, t, stream);
    });
}
