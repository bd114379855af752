// General filter-bank 2-D DWT / IDWT, one level per launch, fp32 (pytorch_wavelets dwt/lowlevel.py:91-172 afb1d, 226-271 sfb1d,
// 312-365 AFB2D, 647-694 SFB2D).  Any even tap count 2 <= L <= 16, separately for the two axes, and the padding modes zero,
// symmetric, reflect, periodic and periodization.  Naming: the "w" bank filters along W (the reference's dim 3 pass, fed with the
// module's *_col buffers), the "h" bank along H (dim 2, the *_row buffers).  Band order of `hi`: (w lo, h hi), (w hi, h lo),
// (w hi, h hi) = the reference's LH, HL, HH.
//
// Analysis  x[NC,H,W] -> ll[NC,OH,OW], hi[NC,3,OH,OW]:   out[i] = sum_k h[k] * xe[2 i + k - base]   along each axis, W first, with
//   base = p / 2, p = 2 (O - 1) - N + L, O = (N + L - 1) / 2           and xe the mode's extension of x     (zero .. periodic)
//   base = L - 1, O = (N + 1) / 2, xe[j] = x[min(((j mod Ne) + L/2) mod Ne, N - 1)] for -Ne <= j < Ne, 0 elsewhere, Ne = N + (N & 1)
//                                                                                                            (periodization:
//   the reference's extend-by-last-sample, roll by -L/2, zero-padded convolution and one wrap-add, folded into one index map).
// A block owns a DA_TH x DA_TW tile of the outputs of one plane: it stages the (2 T + L - 2)-sided input patch in LDS through the
// index map, runs the W pass for every patch row (lo and hi, into LDS), then the H pass, and stores the four bands.  x is read
// once (plus the halo), every band written once, nothing intermediate leaves the CU.  The taps travel by value in the kernel
// arguments: no device allocation, no copy, no state -- the launch can be captured in a graph.  Every output is a fixed-order sum
// (k = 0 .. L-1 per pass), whatever the tile it falls in: bit-reproducible.
//
// Synthesis  ll, hi (either may be NULL = zeros) [NC,nh,nw] -> y[NC,out_h,out_w], the top-left crop of the full result:
//   full[m] = sum_i lo[i] g0[m - 2 i] + hi[i] g1[m - 2 i]                              (transposed stride-2 bank), H first, then W
//   y[t] = full[t + L - 2],                       0 <= t < 2 n - L + 2                  (zero .. periodic)
//   y[t] = w[(t + L/2 - 1) mod 2n],  w[u] = full[u] + (u < L - 2 ? full[u + 2n] : 0)   (periodization: wrap-add, then the roll).
// With u' = t + L/2 - 1 (not wrapped) and a virtual coefficient index i' that wraps (c[i' mod n]) the periodization sum is the
// same transposed bank over i' in [-n, n) for u' < 2n and over [0, 2n) for u' >= 2n; the other modes use i' in [0, n).  A block
// owns a DS_TH x DS_TW tile of y, stages the (T/2 + L/2)-sided patch of the four bands, runs the H pass into LDS and the W pass
// into y.  AFB2D.backward is this kernel on the analysis taps with the crop, SFB2D.backward the analysis kernel on the synthesis
// taps: the reference defines its backward passes that way (they are the adjoint only for zero padding, and for periodization
// at even sizes).
#include <cstdint>
#include "filterbank_dev.h"

namespace faoctasr {

constexpr int DA_TH = 16, DA_TW = 32;                       // analysis: output tile
constexpr int DA_PR = 2 * DA_TH + FB_MAXL - 2;             // patch rows
constexpr int DA_PC = 2 * DA_TW + FB_MAXL - 2;             // patch columns (even: the W pass reads aligned float2)
constexpr int DS_TH = 32, DS_TW = 64;                       // synthesis: output tile
constexpr int DS_PR = DS_TH / 2 + FB_MAXL / 2;             // coefficient patch rows
constexpr int DS_PC = DS_TW / 2 + FB_MAXL / 2;             // coefficient patch columns

__global__ __launch_bounds__(256) void dwt_analysis_kernel(const float* __restrict__ x, float* __restrict__ ll, float* __restrict__ hi,
                                                           int H, int W, int OH, int OW, int tiles_h, int tiles_w, int Lh, int Lw,
                                                           int base_h, int base_w, int mode, FbTaps2 taps) {
    __shared__ __attribute__((aligned(16))) float patch[DA_PR][DA_PC];
    __shared__ float mid_lo[DA_PR][DA_TW], mid_hi[DA_PR][DA_TW];
    const int tid = threadIdx.x;
    const PlaneTile t = plane_tile<DA_TH, DA_TW>(tiles_h, tiles_w);
    const long plane = t.plane;
    const int oi0 = t.y0, oj0 = t.x0;
    const int rows = 2 * DA_TH + Lh - 2, cols = 2 * DA_TW + Lw - 2;      // <= DA_PR, DA_PC
    const float* xp = x + plane * H * (long)W;

    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = fb_map(2 * oi0 - base_h + r, H, mode, Lh >> 1);
        for (int c = tid & 63; c < cols; c += 64) {
            const int sc = fb_map(2 * oj0 - base_w + c, W, mode, Lw >> 1);
            patch[r][c] = (sr >= 0 && sc >= 0) ? xp[(long)sr * W + sc] : 0.f;
        }
    }
    __syncthreads();

    {   // W pass: thread (r, c) filters patch row r at output column c
        const int c = tid & 31;
        for (int r = tid >> 5; r < rows; r += 8) {
            float lo = 0.f, hv = 0.f;
            for (int k = 0; k < Lw; k += 2) {
                const float2 v = *reinterpret_cast<const float2*>(&patch[r][2 * c + k]);
                lo = fmaf(taps.w.f0[k], v.x, lo);
                hv = fmaf(taps.w.f1[k], v.x, hv);
                lo = fmaf(taps.w.f0[k + 1], v.y, lo);
                hv = fmaf(taps.w.f1[k + 1], v.y, hv);
            }
            mid_lo[r][c] = lo;
            mid_hi[r][c] = hv;
        }
    }
    __syncthreads();

    {   // H pass
        const int c = tid & 31;
        const int oj = oj0 + c;
        const long band = (long)OH * OW;
        float* llp = ll + plane * band;
        float* hip_ = hi + plane * 3 * band;
        for (int i = tid >> 5; i < DA_TH; i += 8) {
            const int oi = oi0 + i;
            float a = 0.f, bb = 0.f, cc = 0.f, d = 0.f;
            for (int k = 0; k < Lh; ++k) {
                const float vl = mid_lo[2 * i + k][c], vh = mid_hi[2 * i + k][c];
                a = fmaf(taps.h.f0[k], vl, a);
                bb = fmaf(taps.h.f1[k], vl, bb);
                cc = fmaf(taps.h.f0[k], vh, cc);
                d = fmaf(taps.h.f1[k], vh, d);
            }
            if (oi < OH && oj < OW) {
                const long o = (long)oi * OW + oj;
                llp[o] = a;
                hip_[o] = bb;
                hip_[band + o] = cc;
                hip_[2 * band + o] = d;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dwt_synthesis_kernel(const float* __restrict__ ll, const float* __restrict__ hi, float* __restrict__ y,
                                                            int nh, int nw, int out_h, int out_w, int tiles_h, int tiles_w, int Lh,
                                                            int Lw, int per, FbTaps2 taps) {
    __shared__ float cf[4][DS_PR][DS_PC];
    __shared__ float mid_lo[DS_TH][DS_PC], mid_hi[DS_TH][DS_PC];
    const int tid = threadIdx.x;
    const PlaneTile tile = plane_tile<DS_TH, DS_TW>(tiles_h, tiles_w);
    const long plane = tile.plane;
    const int t0 = tile.y0, s0 = tile.x0;
    const int off_h = per ? (Lh >> 1) - 1 : Lh - 2, off_w = per ? (Lw >> 1) - 1 : Lw - 2;
    const int ib = (t0 + off_h - Lh + 2) >> 1, jb = (s0 + off_w - Lw + 2) >> 1;     // first virtual coefficient row / column (floor)
    const int prow = DS_TH / 2 + (Lh >> 1), pcol = DS_TW / 2 + (Lw >> 1);
    const long band = (long)nh * nw;
    const float* llp = ll ? ll + plane * band : nullptr;
    const float* hp = hi ? hi + plane * 3 * band : nullptr;

    for (int r = tid >> 6; r < prow; r += 4) {
        const int sr = pmod(ib + r, nh);
        for (int c = tid & 63; c < pcol; c += 64) {
            const long o = (long)sr * nw + pmod(jb + c, nw);
            cf[0][r][c] = llp ? llp[o] : 0.f;
            cf[1][r][c] = hp ? hp[o] : 0.f;
            cf[2][r][c] = hp ? hp[band + o] : 0.f;
            cf[3][r][c] = hp ? hp[2 * band + o] : 0.f;
        }
    }
    __syncthreads();

    // H pass: (ll, lh) -> mid_lo, (hl, hh) -> mid_hi, for every row of the tile and every patch column: fb_syn_out's loop, written
    // out for two outputs that share the taps and the index (two calls cost four VGPRs)
    for (int e = tid; e < DS_TH * pcol; e += 256) {
        const int tt = e / pcol, c = e - tt * pcol;
        const int u = t0 + tt + off_h;
        const int lo_i = (per && u < 2 * nh) ? -nh : 0, hi_i = (per && u >= 2 * nh) ? 2 * nh : nh;
        const bool odd = u & 1;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        for (int q = 0; q < (Lh >> 1); ++q) {
            const int i = (u >> 1) - q;
            if (i < lo_i || i >= hi_i) continue;
            const float g0 = odd ? taps.h.f0[2 * q + 1] : taps.h.f0[2 * q], g1 = odd ? taps.h.f1[2 * q + 1] : taps.h.f1[2 * q];
            const int r = i - ib;
            a0 = fmaf(cf[0][r][c], g0, a0);
            a1 = fmaf(cf[1][r][c], g1, a1);
            b0 = fmaf(cf[2][r][c], g0, b0);
            b1 = fmaf(cf[3][r][c], g1, b1);
        }
        mid_lo[tt][c] = a0 + a1;
        mid_hi[tt][c] = b0 + b1;
    }
    __syncthreads();

    float* yp = y + plane * out_h * (long)out_w;
    for (int e = tid; e < DS_TH * DS_TW; e += 256) {
        const int tt = e / DS_TW, ss = e - tt * DS_TW;
        const int t = t0 + tt, s = s0 + ss;
        if (t >= out_h || s >= out_w) continue;
        yp[(long)t * out_w + s] = fb_syn_out(mid_lo[tt], mid_hi[tt], jb, nw, s + off_w, per, Lw, taps.w);
    }
}

static int mode_ok(int mode) {
    return mode == MODE_ZERO || mode == MODE_SYMMETRIC || mode == MODE_PER || mode == MODE_REFLECT || mode == MODE_PERIODIC;
}

static int dwt_check(const char* what, long NC, int L_h, int L_w, int mode, const float* a, const float* b, const float* c, const float* d) {
    if (int rc = fb_check2(what, NC, L_h, L_w, a, b, c, d)) return rc;
    if (!mode_ok(mode)) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d (0 zero, 1 symmetric, 2 periodization, 4 reflect, 6 periodic)", what, mode);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

static int dwt_out_size(int N, int L, int mode) {
    return mode == MODE_PER ? (N + 1) / 2 : (N + L - 1) / 2;
}

extern "C" int faoctasr_dwt2d_analysis(const float* x, float* ll, float* hi, long NC, int H, int W, const float* lo_h, const float* hi_h,
                                       int L_h, const float* lo_w, const float* hi_w, int L_w, int mode, faoctasr_stream_t stream) {
    int rc = dwt_check("dwt2d_analysis", NC, L_h, L_w, mode, lo_h, hi_h, lo_w, hi_w);
    if (rc) return rc;
    if (!x || !ll || !hi) return fail(FAOCTASR_EINVAL, "dwt2d_analysis: null pointer");
    if (H < L_h / 2 + 1 || W < L_w / 2 + 1)
        return fail(FAOCTASR_EINVAL, "dwt2d_analysis: H %d W %d below the minimum side L/2 + 1 (L_h %d, L_w %d)", H, W, L_h, L_w);
    const int OH = dwt_out_size(H, L_h, mode), OW = dwt_out_size(W, L_w, mode);
    int tiles_h, tiles_w;
    long blocks;
    if (!plane_tiles(NC, OH, OW, DA_TH, DA_TW, &tiles_h, &tiles_w, &blocks)) return fail(FAOCTASR_EUNSUPPORTED, "dwt2d_analysis: NC %ld H %d W %d needs more than 2^31 - 1 blocks", NC, H, W);
    const int base_h = mode == MODE_PER ? L_h - 1 : (2 * (OH - 1) - H + L_h) / 2;
    const int base_w = mode == MODE_PER ? L_w - 1 : (2 * (OW - 1) - W + L_w) / 2;
    hipLaunchKernelGGL(dwt_analysis_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ll, hi, H, W, OH, OW, tiles_h,
                       tiles_w, L_h, L_w, base_h, base_w, mode, fb_taps2(lo_h, hi_h, L_h, lo_w, hi_w, L_w));
    return check_launch("dwt2d_analysis");
}

extern "C" int faoctasr_dwt2d_synthesis(const float* ll, const float* hi, float* y, long NC, int nh, int nw, int out_h, int out_w,
                                        const float* lo_h, const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w,
                                        int mode, faoctasr_stream_t stream) {
    int rc = dwt_check("dwt2d_synthesis", NC, L_h, L_w, mode, lo_h, hi_h, lo_w, hi_w);
    if (rc) return rc;
    if (!y) return fail(FAOCTASR_EINVAL, "dwt2d_synthesis: null output pointer");
    const int per = mode == MODE_PER;
    // a result of at least one sample (2 n - L + 2 >= 2), resp. a periodization roll of at most one turn (2 n >= L / 2)
    if (nh < (per ? (L_h + 3) / 4 : L_h / 2) || nw < (per ? (L_w + 3) / 4 : L_w / 2))
        return fail(FAOCTASR_EINVAL, "dwt2d_synthesis: coefficient size %d x %d below the minimum side (L_h %d, L_w %d)", nh, nw, L_h, L_w);
    const int full_h = per ? 2 * nh : 2 * nh - L_h + 2, full_w = per ? 2 * nw : 2 * nw - L_w + 2;
    if (out_h < 1 || out_w < 1 || out_h > full_h || out_w > full_w)
        return fail(FAOCTASR_EINVAL, "dwt2d_synthesis: crop %d x %d outside the %d x %d result", out_h, out_w, full_h, full_w);
    int tiles_h, tiles_w;
    long blocks;
    if (!plane_tiles(NC, out_h, out_w, DS_TH, DS_TW, &tiles_h, &tiles_w, &blocks)) return fail(FAOCTASR_EUNSUPPORTED, "dwt2d_synthesis: NC %ld, %d x %d needs more than 2^31 - 1 blocks", NC, out_h, out_w);
    hipLaunchKernelGGL(dwt_synthesis_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ll, hi, y, nh, nw, out_h, out_w,
                       tiles_h, tiles_w, L_h, L_w, per, fb_taps2(lo_h, hi_h, L_h, lo_w, hi_w, L_w));
    return check_launch("dwt2d_synthesis");
}
