// Stationary (undecimated, a-trous) 2-D wavelet transform, one level per launch, fp32 (pytorch_wavelets dwt/lowlevel.py:175-223
// afb1d_atrous, 475-521 afb2d_atrous; transform2d.py:151-212 SWTForward).  Any even tap count 2 <= L <= 16, separately for the two
// axes, dilation d = 2^level in {1, 2, 4, 8}, and the extensions zero, symmetric, reflect and periodic.  Naming, as SWTForward
// hands its buffers to afb2d_atrous: the "h" bank filters along H (dim 2, the module's *_col buffers), the "w" bank along W
// (dim 3, *_row) -- NOT the swapped mapping of dwt.hip.  The taps are in wavelet order (dec_lo / dec_hi, not the reversed buffers).
//
// Analysis  x[NC planes of H x W, plane stride xps] -> y[NC,4,H,W], per axis, W first:
//     out[i] = sum_k h[k] * xe[i - k d + L d / 2],         xe the mode's extension of x,
// band 0 = (w lo, h lo), 1 = (w lo, h hi), 2 = (w hi, h lo), 3 = (w hi, h hi).  Output i touches only samples congruent to
// i + L d / 2 (mod d), so a block owns SA_TH output rows of ONE residue class mod d along H (a patch of SA_TH + L - 1 rows,
// whatever d) and SA_TW contiguous output columns (a patch of SA_TW + (L - 1) d columns: global reads stay contiguous).  It
// stages the patch in LDS through the extension's index map, runs the W pass for every patch row (lo and hi, into LDS), then
// the H pass, and stores the four bands: x is read once (plus the halo), each band written once.  The plane stride lets level
// j + 1 read band 0 of level j's output in place.
//
// Adjoint  c[NC,4,H,W] -> dx[NC planes, plane stride dps], the transpose of the analysis in all four modes:
//     dx[j] = sum_{p : map(p) = j} sum_k h[k] * c0[p + k d - L d / 2],      c0 = c inside [0, N), zero outside,
// the H axis first (bands (0, 1) -> lo, (2, 3) -> hi), then W.  An optional plane `band0` is added to band 0 of c as it is read
// (the coarser level's gradient joining a level's cotangent) or read in its place (the coarser level's reconstruction standing
// in for a level's own lowpass): the levels chain without a copy of the coefficients.  p need not be restricted to the extended domain
// [-(L d / 2 - d), N + L d / 2): an index p + k d - L d / 2 inside [0, N) puts p inside it.  Under the geometry rule
// N >= L d / 2 + 1 the extension folds at most once a side, so a sample has at most three preimages -- itself and one mirror or
// wrap per side -- summed in that fixed order, each over k = 0 .. L-1: a gather, no atomics.  For 'periodic' the three collapse
// into one sum over the wrapped index.  A block owns the same tile shape as the analysis.  Its H pass reads c from global memory
// (coalesced along W; the mirrored rows of a folding mode belong to other residue classes, which an LDS patch of one class
// would not hold) for the SJ_TW + L d columns the W pass can touch -- the mirrored columns of an output lie within L d / 2 of it
// -- and leaves the two half-sums in LDS; the W pass gathers from there.  Each coefficient comes from HBM once (plus the halo;
// the H pass's L-fold re-reads are cache hits), dx is written once, nothing intermediate leaves the CU.
//
// The periodic inverse (iswt2's, per level and axis y[m] = 1/2 sum_k g0[k] lo[(m - k d + (L/2 - 1) d) mod N] + g1[k] hi[same])
// is the adjoint kernel on the reversed rec taps with scale 1/4, and its backward the analysis kernel on those taps and scale.
// The taps travel by value in the kernel arguments: no device allocation, no copy, no state -- the launches can be captured in
// a graph.  Every output is a fixed-order sum whatever the tile it falls in: bit-reproducible.
#include <cstdint>
#include "filterbank_dev.h"

namespace faoctasr {

constexpr int SWT_MAXD = 8;

constexpr int SA_TH = 16, SA_TW = 64;                           // analysis: output tile (rows of one residue class, columns)
constexpr int SA_PR = SA_TH + FB_MAXL - 1;                     // patch rows
constexpr int SA_PC = SA_TW + (FB_MAXL - 1) * SWT_MAXD;        // patch columns
constexpr int SJ_TH = 16, SJ_TW = 64;                           // adjoint: output tile
constexpr int SJ_PC = SJ_TW + FB_MAXL * SWT_MAXD;              // columns of the H pass's half-sums

__global__ __launch_bounds__(256) void swt_analysis_kernel(const float* __restrict__ x, long xps, float* __restrict__ y, int H, int W, int d,
                                                           int tiles_h, int tiles_w, int Lh, int Lw, int mode, float scale, FbTaps2 taps) {
    __shared__ float patch[SA_PR][SA_PC];
    __shared__ float mid_lo[SA_PR][SA_TW], mid_hi[SA_PR][SA_TW];
    const int tid = threadIdx.x;
    long b = blockIdx.x;
    const int tw = (int)(b % tiles_w); b /= tiles_w;
    const int th = (int)(b % tiles_h); b /= tiles_h;
    const int r = (int)(b % d);
    const long plane = b / d;
    const int t0 = th * SA_TH, j0 = tw * SA_TW;
    if (r + (long)d * t0 >= H) return;                                  // a residue class with fewer rows than the others
    const int rows = SA_TH + Lh - 1, cols = SA_TW + (Lw - 1) * d;       // <= SA_PR, SA_PC
    const float* xp = x + plane * xps;

    // patch row q holds extended row r + d (t0 + q - Lh/2 + 1), patch column c extended column j0 + c - (Lw/2 - 1) d
    for (int c = tid & 63; c < cols; c += 64) {
        const int sc = fb_map(j0 + c - ((Lw >> 1) - 1) * d, W, mode, 0);
        for (int q = tid >> 6; q < rows; q += 4) {
            const int sr = fb_map(r + d * (t0 + q - (Lh >> 1) + 1), H, mode, 0);
            patch[q][c] = (sr >= 0 && sc >= 0) ? xp[(long)sr * W + sc] : 0.f;
        }
    }
    __syncthreads();

    const int jj = tid & 63;
    for (int q = tid >> 6; q < rows; q += 4) {                          // W pass: output column jj, tap k reads column jj + (Lw-1-k) d
        float lo = 0.f, hv = 0.f;
        for (int k = 0; k < Lw; ++k) {
            const float v = patch[q][jj + (Lw - 1 - k) * d];
            lo = fmaf(taps.w.f0[k], v, lo);
            hv = fmaf(taps.w.f1[k], v, hv);
        }
        mid_lo[q][jj] = lo;
        mid_hi[q][jj] = hv;
    }
    __syncthreads();

    const int j = j0 + jj;
    const long band = (long)H * W;
    float* yp = y + plane * 4 * band;
    for (int t = tid >> 6; t < SA_TH; t += 4) {                         // H pass: output row t of the class, tap k reads row t + Lh-1-k
        const long i = r + (long)d * (t0 + t);
        float a = 0.f, bb = 0.f, cc = 0.f, dd = 0.f;
        for (int k = 0; k < Lh; ++k) {
            const float vl = mid_lo[t + Lh - 1 - k][jj], vh = mid_hi[t + Lh - 1 - k][jj];
            a = fmaf(taps.h.f0[k], vl, a);
            bb = fmaf(taps.h.f1[k], vl, bb);
            cc = fmaf(taps.h.f0[k], vh, cc);
            dd = fmaf(taps.h.f1[k], vh, dd);
        }
        if (i < H && j < W) {
            const long o = i * W + j;
            yp[o] = a * scale;
            yp[band + o] = bb * scale;
            yp[2 * band + o] = cc * scale;
            yp[3 * band + o] = dd * scale;
        }
    }
}

// the two half-sums of the adjoint's H pass at row p (any integer) and column sc: taps k = 0 .. Lh-1 over the rows p + (k - Lh/2) d
// that fall inside the image (wrap: taken mod H).  Band 0 is c's own (own0, NULL when replaced) plus the extra plane x0 (NULL: none)
__device__ __forceinline__ void swt_adj_rows(const float* __restrict__ cp, const float* __restrict__ own0, const float* __restrict__ x0, long band,
                                             int W, int H, int p, int sc, int d, int Lh, bool wrap, const FbTaps2& taps, float& lo, float& hv) {
    for (int k = 0; k < Lh; ++k) {
        int e = p + (k - (Lh >> 1)) * d;
        if (wrap) e = pmod(e, H);
        if (e < 0 || e >= H) continue;
        const long o = (long)e * W + sc;
        float v = own0 ? own0[o] : 0.f;
        if (x0) v += x0[o];
        lo = fmaf(taps.h.f0[k], v, lo);
        lo = fmaf(taps.h.f1[k], cp[band + o], lo);
        hv = fmaf(taps.h.f0[k], cp[2 * band + o], hv);
        hv = fmaf(taps.h.f1[k], cp[3 * band + o], hv);
    }
}

// the adjoint's W pass for preimage column p: taps over the virtual columns p + (k - Lw/2) d, read from the half-sums whose
// column 0 is virtual column v0 (the half-sums of a column outside the image are zero in the folding modes, so a mirrored
// preimage needs no clipping to the image, only to the staged columns)
__device__ __forceinline__ float swt_adj_cols(const float* __restrict__ lo, const float* __restrict__ hv, int p, int v0, int d, int Lw,
                                              const FbTaps2& taps, float acc) {
    for (int k = 0; k < Lw; ++k) {
        const int m = p + (k - (Lw >> 1)) * d - v0;
        if (m < 0 || m >= SJ_PC) continue;
        acc = fmaf(taps.w.f0[k], lo[m], acc);
        acc = fmaf(taps.w.f1[k], hv[m], acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void swt_adjoint_kernel(const float* __restrict__ c, float* __restrict__ dx, long dps,
                                                          const float* __restrict__ band0, long b0ps, int band0_replaces, int H, int W, int d,
                                                          int tiles_h, int tiles_w, int Lh, int Lw, int mode, float scale, FbTaps2 taps) {
    __shared__ float mid_lo[SJ_TH][SJ_PC], mid_hi[SJ_TH][SJ_PC];
    const int tid = threadIdx.x;
    long b = blockIdx.x;
    const int tw = (int)(b % tiles_w); b /= tiles_w;
    const int th = (int)(b % tiles_h); b /= tiles_h;
    const int r = (int)(b % d);
    const long plane = b / d;
    const int t0 = th * SJ_TH, j0 = tw * SJ_TW;
    if (r + (long)d * t0 >= H) return;
    const long band = (long)H * W;
    const float* cp = c + plane * 4 * band;
    const float* x0 = band0 ? band0 + plane * b0ps : nullptr;          // joins band 0 of c, or stands in for it
    const float* own0 = (band0 && band0_replaces) ? nullptr : cp;
    const bool wrap = mode == MODE_PERIODIC, fold = mode == MODE_SYMMETRIC || mode == MODE_REFLECT;
    const int off = mode == MODE_SYMMETRIC ? 1 : 0;                      // mirrors of j: -off - j and 2 N - 2 + off - j
    const int v0 = j0 - (Lw >> 1) * d;                                  // virtual column of half-sum column 0
    const int cols = SJ_TW + Lw * d;                                    // <= SJ_PC

    for (int m = tid & 63; m < SJ_PC; m += 64) {                        // H pass (columns past `cols` are cleared, never read)
        const int v = v0 + m;
        const int sc = m < cols ? (wrap ? pmod(v, W) : (v >= 0 && v < W ? v : -1)) : -1;
        for (int t = tid >> 6; t < SJ_TH; t += 4) {
            const long jl = r + (long)d * (t0 + t);
            float lo = 0.f, hv = 0.f;
            if (sc >= 0 && jl < H) {
                const int j = (int)jl;
                swt_adj_rows(cp, own0, x0, band, W, H, j, sc, d, Lh, wrap, taps, lo, hv);
                if (fold) {
                    if (j >= 1 - off && j < (Lh >> 1) * d) swt_adj_rows(cp, own0, x0, band, W, H, -off - j, sc, d, Lh, false, taps, lo, hv);
                    if (j <= H - 2 + off && j >= H - 1 - (Lh >> 1) * d)
                        swt_adj_rows(cp, own0, x0, band, W, H, 2 * H - 2 + off - j, sc, d, Lh, false, taps, lo, hv);
                }
            }
            mid_lo[t][m] = lo;
            mid_hi[t][m] = hv;
        }
    }
    __syncthreads();

    const int jj = tid & 63, j = j0 + jj;
    if (j >= W) return;
    float* dp = dx + plane * dps;
    for (int t = tid >> 6; t < SJ_TH; t += 4) {                         // W pass
        const long i = r + (long)d * (t0 + t);
        if (i >= H) break;
        float acc = swt_adj_cols(mid_lo[t], mid_hi[t], j, v0, d, Lw, taps, 0.f);
        if (fold) {
            if (j >= 1 - off && j < (Lw >> 1) * d) acc = swt_adj_cols(mid_lo[t], mid_hi[t], -off - j, v0, d, Lw, taps, acc);
            if (j <= W - 2 + off && j >= W - 1 - (Lw >> 1) * d)
                acc = swt_adj_cols(mid_lo[t], mid_hi[t], 2 * W - 2 + off - j, v0, d, Lw, taps, acc);
        }
        dp[i * W + j] = acc * scale;
    }
}

static int swt_check(const char* what, long NC, int H, int W, long plane_stride, int L_h, int L_w, int dilation, int mode, const float* a,
                     const float* b, const float* c, const float* d) {
    if (int rc = fb_check2(what, NC, L_h, L_w, a, b, c, d)) return rc;
    if (mode != MODE_ZERO && mode != MODE_SYMMETRIC && mode != MODE_REFLECT && mode != MODE_PERIODIC)
        return fail(FAOCTASR_EINVAL, "%s: unknown extension %d (0 zero, 1 symmetric, 4 reflect, 6 periodic)", what, mode);
    if (dilation != 1 && dilation != 2 && dilation != 4 && dilation != SWT_MAXD)
        return fail(FAOCTASR_EINVAL, "%s: dilation %d is not one of 1, 2, 4, %d", what, dilation, SWT_MAXD);
    if (H < L_h * dilation / 2 + 1 || W < L_w * dilation / 2 + 1)
        return fail(FAOCTASR_EINVAL, "%s: H %d W %d below the minimum side L d / 2 + 1 (L_h %d, L_w %d, dilation %d)", what, H, W, L_h, L_w,
                    dilation);
    if (plane_stride < (long)H * W) return fail(FAOCTASR_EINVAL, "%s: plane stride %ld below H W = %ld", what, plane_stride, (long)H * W);
    return FAOCTASR_OK;
}

// blocks of one launch: planes x residue classes x tiles of the largest class x column tiles; 0 when that passes 2^31 - 1
static long swt_blocks(long NC, int H, int W, int d, int TH, int TW, int* tiles_h, int* tiles_w) {
    *tiles_h = ((H + d - 1) / d + TH - 1) / TH;
    *tiles_w = (W + TW - 1) / TW;
    const long per_plane = (long)d * *tiles_h * *tiles_w;
    if (NC > 0x7fffffffL / per_plane) return 0;
    return NC * per_plane;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" int faoctasr_swt2d_analysis(const float* x, long x_plane_stride, float* y, long NC, int H, int W, const float* lo_h,
                                       const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w, int dilation, int mode,
                                       float scale, faoctasr_stream_t stream) {
    int rc = swt_check("swt2d_analysis", NC, H, W, x_plane_stride, L_h, L_w, dilation, mode, lo_h, hi_h, lo_w, hi_w);
    if (rc) return rc;
    if (!x || !y) return fail(FAOCTASR_EINVAL, "swt2d_analysis: null pointer");
    int tiles_h, tiles_w;
    const long blocks = swt_blocks(NC, H, W, dilation, SA_TH, SA_TW, &tiles_h, &tiles_w);
    if (!blocks) return fail(FAOCTASR_EUNSUPPORTED, "swt2d_analysis: NC %ld H %d W %d needs more than 2^31 - 1 blocks", NC, H, W);
    hipLaunchKernelGGL(swt_analysis_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_plane_stride, y, H, W, dilation,
                       tiles_h, tiles_w, L_h, L_w, mode, scale, fb_taps2(lo_h, hi_h, L_h, lo_w, hi_w, L_w));
    return check_launch("swt2d_analysis");
}

extern "C" int faoctasr_swt2d_adjoint(const float* c, float* dx, long dx_plane_stride, const float* band0, long band0_plane_stride,
                                      int band0_replaces, long NC, int H, int W, const float* lo_h,
                                      const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w, int dilation, int mode,
                                      float scale, faoctasr_stream_t stream) {
    int rc = swt_check("swt2d_adjoint", NC, H, W, dx_plane_stride, L_h, L_w, dilation, mode, lo_h, hi_h, lo_w, hi_w);
    if (rc) return rc;
    if (!c || !dx) return fail(FAOCTASR_EINVAL, "swt2d_adjoint: null pointer");
    if (band0 && band0_plane_stride < (long)H * W)
        return fail(FAOCTASR_EINVAL, "swt2d_adjoint: band-0 plane stride %ld below H W = %ld", band0_plane_stride, (long)H * W);
    int tiles_h, tiles_w;
    const long blocks = swt_blocks(NC, H, W, dilation, SJ_TH, SJ_TW, &tiles_h, &tiles_w);
    if (!blocks) return fail(FAOCTASR_EUNSUPPORTED, "swt2d_adjoint: NC %ld H %d W %d needs more than 2^31 - 1 blocks", NC, H, W);
    hipLaunchKernelGGL(swt_adjoint_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, c, dx, dx_plane_stride, band0, band0_plane_stride, band0_replaces, H, W, dilation,
                       tiles_h, tiles_w, L_h, L_w, mode, scale, fb_taps2(lo_h, hi_h, L_h, lo_w, hi_w, L_w));
    return check_launch("swt2d_adjoint");
}
