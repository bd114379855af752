// DTCWT magnitude loss, fp32: for two images x, y of shape (N, C, H, W)
//
//   L(x, y) = sum_{j = 1..J} w_j * mean_{n, c, o, h, w} | r_j(x) - r_j(y) |,     r = sqrt(re^2 + im^2 + b^2)
//
// over the six complex bandpass orientations of every level of the dual-tree transform (dtcwt.hip); no lowpass term.  r is the
// smoothed magnitude of the scattering layers (scat.hip) with its bias b, which cancels in the difference.
//
// The two analysis kernels run the forward tile bodies of dtcwt_dev.h, as dtcwt_fwd_j1 / dtcwt_fwd_j2 do (two-filter form), every
// block twice through the SAME LDS: its tile of x, then its tile of y.  The loop over the two images is not unrolled, so
// both run one instruction sequence (L(x, y) and L(y, x) agree bit for bit); x's complex values wait in registers while y's are
// computed.  In the place of the bandpass stores:
//   - one partial sum of |r_x - r_y| per block into `part`: per-thread sum (orientations in a fixed order), a 64-lane butterfly,
//     then the four waves -- no atomics;
//   - where gx (gy) is not null, the cotangent band of x (y): sign(r_x - r_y) * z_x / r_x * scale (the negative, with z_y / r_y),
//     scale = w_j / count_j, one float2 per coefficient of a contiguous (N, C, 6, h, w, 2) tensor; sign(0) = 0.  The transform's
//     adjoint (dtcwt_inv_j2 / dtcwt_inv_j1 on the analysis taps) turns these into dL/dx: the backward has no kernel of its own;
//   - where llx (lly) is not null, the level's lowpass for the next level (null at the last level), contiguous.
// Threads of remainder tiles (`live` false) contribute zero and store nothing.
//
// A last single-block kernel adds every level's partials in a fixed order in double, applies w_j / count_j and writes the float.
// Taps travel by value, nothing is allocated, no state: capturable and bit-reproducible.
#include "dtcwt_dev.h"

namespace faoctasr {

constexpr int DL_MAXJ = 16;                       // levels of one loss (a side of 2^16 at the least)

struct DlLevels { long n[DL_MAXJ]; double s[DL_MAXJ]; };                 // per level: partials, w_j / count_j

// |r_x - r_y| of one orientation, and its two cotangents
__device__ __forceinline__ float dl_term(float2 zx, float2 zy, float b2, float scale, float2* gx, float2* gy) {
    const float rx = sqrtf(zx.x * zx.x + zx.y * zx.y + b2), ry = sqrtf(zy.x * zy.x + zy.y * zy.y + b2);
    const float d = rx - ry;
    const float sg = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);
    if (gx) *gx = make_float2(zx.x / rx * sg, zx.y / rx * sg);
    if (gy) *gy = make_float2(zy.x / ry * -sg, zy.y / ry * -sg);
    return fabsf(d);
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1: x, y [H, W] even -> ll of each [H, W] (optional), cotangent bands [H/2, W/2] (optional), one partial per block
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dtcwt_loss_fwd_j1(const float* __restrict__ x, DtLow xs, const float* __restrict__ y, DtLow ys,
                                                         float* __restrict__ llx, float* __restrict__ lly, float2* __restrict__ gx,
                                                         float2* __restrict__ gy, float* __restrict__ part, float scale, float b2, int C,
                                                         int H, int W, int tiles_h, int tiles_w, int L0, int L1, int sym, DtTaps1 taps) {
    __shared__ float patch[J1_PR][J1_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[J1_PR][J1_TW];
    __shared__ float red[4];
    const DtTile t = dt_tile(tiles_h, tiles_w);
    const long plane = t.plane, n = plane / C, c = plane % C;
    const int oi0 = t.th * J1_TH, oj0 = t.tw * J1_TW;
    const int qi = threadIdx.x >> 5, qj = threadIdx.x & 31;               // H pass: a thread owns one 2x2 quad of the tile
    const int oi = oi0 + 2 * qi, oj = oj0 + 2 * qj;
    const bool live = oi < H && oj < W;                                   // H, W even: a quad is inside or outside as a whole
    float2 z[6], zx[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) z[o] = zx[o] = make_float2(0.f, 0.f);

#pragma unroll 1
    for (int img = 0; img < 2; ++img) {                                   // one instruction sequence for both images
        float* ll = img ? lly : llx;
        dt_fwd1_rows<true, false>(img ? y + n * ys.n + c * ys.c : x + n * xs.n + c * xs.c, img ? ys.r : xs.r, oi0, oj0, H, W, sym, L0, L1, taps,
                                  patch, mid_lo, mid_hi, nullptr);
        if (live) {
            const DtQuad1 v = dt_fwd1_quad<true, false>(qi, qj, L0, L1, taps, mid_lo, mid_hi, nullptr);
            if (ll) {
                float* lp = ll + plane * H * (long)W + (long)oi * W + oj;
                *reinterpret_cast<float2*>(lp) = v.ll[0];
                *reinterpret_cast<float2*>(lp + W) = v.ll[1];
            }
            dt_q2c_val(v.lh[0], v.lh[1], &z[0], &z[5]);
            dt_q2c_val(v.hh[0], v.hh[1], &z[1], &z[4]);
            dt_q2c_val(v.hl[0], v.hl[1], &z[2], &z[3]);
        }
        if (img == 0) {
#pragma unroll
            for (int o = 0; o < 6; ++o) zx[o] = z[o];
        }
    }

    float acc = 0.f;
    if (live) {
        const long hw = (long)(H >> 1) * (W >> 1), at = (long)(oi >> 1) * (W >> 1) + (oj >> 1);
#pragma unroll
        for (int o = 0; o < 6; ++o) {
            const long e = (plane * 6 + o) * hw + at;
            acc += dl_term(zx[o], z[o], b2, scale, gx ? gx + e : nullptr, gy ? gy + e : nullptr);
        }
    }
    block_partial_store_256(acc, red, part);
}

// ---------------------------------------------------------------------------------------------------------------------------
// level >= 2: x, y [H, W] (multiples of 4) -> ll of each [H/2, W/2] (optional), cotangent bands [H/4, W/4] (optional), partials
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dtcwt_loss_fwd_j2(const float* __restrict__ x, DtLow xs, const float* __restrict__ y, DtLow ys,
                                                         float* __restrict__ llx, float* __restrict__ lly, float2* __restrict__ gx,
                                                         float2* __restrict__ gy, float* __restrict__ part, float scale, float b2, int C,
                                                         int H, int W, int tiles_h, int tiles_w, int m, DtTaps2 taps) {
    __shared__ __attribute__((aligned(16))) float patch[F2_PR][F2_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[F2_PR][F2_TW];
    __shared__ float red[4];
    const DtTile t = dt_tile(tiles_h, tiles_w);
    const long plane = t.plane, n = plane / C, c = plane % C;
    const int OH = H >> 1, OW = W >> 1, BH = H >> 2, BW = W >> 2;          // of ll; of the bands
    const int i0 = t.th * (F2_TH / 2), j0 = t.tw * (F2_TW / 2);           // first quad row / column = first index of the trees
    const int tid = threadIdx.x, path = tid >> 7, qi = (tid & 127) >> 5, qj = tid & 31;
    const int pi = i0 + qi, pj = j0 + qj;
    const bool live = pi < BH && pj < BW;
    float2 z[4], zx[4];                                                   // path 0: lh z1, z2 (15, 165); path 1: hl z1, z2 (75, 105), hh z1, z2 (45, 135)
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = zx[k] = make_float2(0.f, 0.f);

#pragma unroll 1
    for (int img = 0; img < 2; ++img) {
        float* ll = img ? lly : llx;
        dt_fwd2_rows<true, false>(img ? y + n * ys.n + c * ys.c : x + n * xs.n + c * xs.c, img ? ys.r : xs.r, i0, j0, H, W, m, taps, patch,
                                  mid_lo, mid_hi, nullptr);
        if (live) {
            const DtQuad2 v = dt_fwd2_quad<true, false>(path, qi, qj, m, taps, mid_lo, mid_hi, nullptr);
            if (path) {
                dt_q2c_val(v.l0, v.l1, &z[0], &z[1]);                     // hl
                dt_q2c_val(v.h0, v.h1, &z[2], &z[3]);                     // hh
            } else {
                if (ll) {
                    float* lp = ll + plane * OH * (long)OW + (long)(2 * pi) * OW + 2 * pj;
                    *reinterpret_cast<float2*>(lp) = v.l0;
                    *reinterpret_cast<float2*>(lp + OW) = v.l1;
                }
                dt_q2c_val(v.h0, v.h1, &z[0], &z[1]);                     // lh
            }
        }
        if (img == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) zx[k] = z[k];
        }
    }

    float acc = 0.f;
    if (live) {
        const long hw = (long)BH * BW, at = (long)pi * BW + pj;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!path && k >= 2) break;
            const int o = path ? (k == 0 ? 2 : k == 1 ? 3 : k == 2 ? 1 : 4) : (k == 0 ? 0 : 5);
            const long e = (plane * 6 + o) * hw + at;
            acc += dl_term(zx[k], z[k], b2, scale, gx ? gx + e : nullptr, gy ? gy + e : nullptr);
        }
    }
    block_partial_store_256(acc, red, part);
}

// the levels' partials lie one after the other in `part`.  Per level: thread t adds partials t, t + 256, ... in double, a fixed
// tree adds the threads, thread 0 applies w_j / count_j and adds the level to the total.
__global__ __launch_bounds__(256) void dtcwt_loss_final_kernel(const float* __restrict__ part, DlLevels lv, int levels, float* __restrict__ out) {
    __shared__ double red[256];
    double total = 0.0;
    long off = 0;
    for (int j = 0; j < levels; ++j) {
        const double s = block_tree_256(strided_sum_256(part + off, lv.n[j]), red);
        if (threadIdx.x == 0) total += s * lv.s[j];
        off += lv.n[j];
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

static int dl_common(const char* what, const void* x, const void* y, const void* part, float scale, float bias2) {
    if (!x || !y || !part) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (!(bias2 > 0.f)) return fail(FAOCTASR_EINVAL, "%s: the squared magnitude bias %g must be positive", what, (double)bias2);
    if (!(scale == scale)) return fail(FAOCTASR_EINVAL, "%s: the scale is not a number", what);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_dtcwt_loss_workspace_floats(long N, int C, int H, int W, int level1) {
    int tiles_h, tiles_w;
    long blocks;
    if (level1 ? dt_tiles1("dtcwt_loss_workspace_floats", H, W, &tiles_h, &tiles_w) : dt_tiles2f("dtcwt_loss_workspace_floats", H, W, &tiles_h, &tiles_w))
        return -1;
    if (dt_blocks("dtcwt_loss_workspace_floats", N, C, tiles_h, tiles_w, &blocks)) return -1;
    return blocks;
}

extern "C" int faoctasr_dtcwt_loss_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, const float* y, long y_sn, long y_sc, long y_sr,
                                          float* llx, float* lly, float* gx, float* gy, float* part, float scale, float bias2, long N,
                                          int C, int H, int W, const float* h0, int L0, const float* h1, int L1, int mode,
                                          faoctasr_stream_t stream) {
    return dt_with_taps1("dtcwt_loss_fwd_j1", h0, L0, h1, L1, nullptr, 0, [&](auto, const DtTaps1& t) {       // two-filter banks only
        int rc, tiles_h, tiles_w;
        if ((rc = dl_common("dtcwt_loss_fwd_j1", x, y, part, scale, bias2))) return rc;
        if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "dtcwt_loss_fwd_j1: unknown padding mode %d", mode);
        if ((rc = dt_tiles1("dtcwt_loss_fwd_j1", H, W, &tiles_h, &tiles_w))) return rc;
        long blocks;
        if ((rc = dt_blocks("dtcwt_loss_fwd_j1", N, C, tiles_h, tiles_w, &blocks))) return rc;
        hipLaunchKernelGGL(dtcwt_loss_fwd_j1, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, DtLow{x_sn, x_sc, x_sr}, y,
                           DtLow{y_sn, y_sc, y_sr}, llx, lly, reinterpret_cast<float2*>(gx), reinterpret_cast<float2*>(gy), part, scale, bias2,
                           C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
        return check_launch("dtcwt_loss_fwd_j1");
    });
}

extern "C" int faoctasr_dtcwt_loss_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, const float* y, long y_sn, long y_sc, long y_sr,
                                          float* llx, float* lly, float* gx, float* gy, float* part, float scale, float bias2, long N,
                                          int C, int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b,
                                          int m, faoctasr_stream_t stream) {
    return dt_with_taps2("dtcwt_loss_fwd_j2", h0a, h0b, h1a, h1b, nullptr, nullptr, m, [&](auto, const DtTaps2& t) {
        int rc, tiles_h, tiles_w;
        if ((rc = dl_common("dtcwt_loss_fwd_j2", x, y, part, scale, bias2))) return rc;
        if ((rc = dt_tiles2f("dtcwt_loss_fwd_j2", H, W, &tiles_h, &tiles_w))) return rc;
        long blocks;
        if ((rc = dt_blocks("dtcwt_loss_fwd_j2", N, C, tiles_h, tiles_w, &blocks))) return rc;
        hipLaunchKernelGGL(dtcwt_loss_fwd_j2, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, DtLow{x_sn, x_sc, x_sr}, y,
                           DtLow{y_sn, y_sc, y_sr}, llx, lly, reinterpret_cast<float2*>(gx), reinterpret_cast<float2*>(gy), part, scale, bias2,
                           C, H, W, tiles_h, tiles_w, m, t);
        return check_launch("dtcwt_loss_fwd_j2");
    });
}

extern "C" int faoctasr_dtcwt_loss_final(const float* workspace, const long* level_floats, const double* level_scale, int levels, float* out,
                                         faoctasr_stream_t stream) {
    if (!workspace || !level_floats || !level_scale || !out) return fail(FAOCTASR_EINVAL, "dtcwt_loss_final: null pointer");
    if (levels < 1 || levels > DL_MAXJ) return fail(FAOCTASR_EINVAL, "dtcwt_loss_final: %d levels, 1..%d are built", levels, DL_MAXJ);
    DlLevels lv = {};
    for (int j = 0; j < levels; ++j) {
        if (level_floats[j] < 1) return fail(FAOCTASR_EINVAL, "dtcwt_loss_final: level %d has %ld partial sums", j + 1, level_floats[j]);
        lv.n[j] = level_floats[j];
        lv.s[j] = level_scale[j];
    }
    hipLaunchKernelGGL(dtcwt_loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, lv, levels, out);
    return check_launch("dtcwt_loss_final");
}
