// Visual information fidelity in the pixel domain (VIFp; Sheikh & Bovik 2006).  Grey planes, fp32.  x is the image under test, r the
// reference, both (N, C, H, W), H, W >= 41, channels independent grey planes pooled inside an image:
//
//   u = (t - lo) * 255 / (hi - lo), value_range = (lo, hi), hi > lo; EPS = 1e-8
//   scale s = 0..3: K_s = 2^(4-s) + 1 (17, 9, 5, 3), w_s[k] = exp(-(k - (K_s-1)/2)^2 / (2 (K_s/5)^2)) / sum; W_s * t the separable VALID convolution
//     s > 0: x_s = (W_s * x_{s-1})[::2, ::2], r_s likewise (the NEW scale's window; rows / columns 0, 2, 4, ...)
//     mx = W_s*x_s, mr = W_s*r_s, sxx = relu(W_s*(x_s x_s) - mx^2), srr = relu(W_s*(r_s r_s) - mr^2), sxr = W_s*(x_s r_s) - mx mr
//     g = sxr / (srr + EPS), sv = sxx - g sxr, then in this order
//       srr < EPS: g = 0, sv = sxx, srr = 0;   sxx < EPS: g = 0, sv = 0;   g < 0: sv = sxx, g = 0;   sv <= EPS: sv = EPS
//     num_s[n] = sum log10(1 + g^2 srr / (sv + sigma_n_sq)), den_s[n] = sum log10(1 + srr / sigma_n_sq) over channels and positions
//   V[n] = (sum_s num_s + EPS) / (sum_s den_s + EPS)
//
// The host computes the taps in double and hands them over by value behind VI_LEAD zeros and before zeros to the end: a strip of
// outputs walks its samples once and multiplies sample k into output j by tap[VI_LEAD + k - j], the zeros taking the places where a
// sample lies outside an output's support (csrc/vessel.hip's scheme).  Every row pass reads LDS sixteen bytes at a time.
//
// vif_scale_fwd: a block takes a 16 x 64 tile of positions, stages the tile plus K_s - 1 rows and columns of both images into LDS
//   (scale 0 through the affine map), runs the row pass into five planes (x, xx, xr, rr, r: 20 FMAs per pair of samples read) and the
//   column pass into registers, four positions of a column per thread, and writes ONE partial of num and one of den per block
//   (per-thread sum, 64-lane butterfly, the four waves in a fixed order: no atomics).  Unless it is the last scale it then filters the
//   staged tile with the next scale's window at the even positions and writes both images of scale s + 1.  The filtered map
//   (side - K_{s+1} + 1) is larger than the stat map (side - K_s + 1): the grid covers the filtered map, and a tile past the stat map
//   skips the statistics and writes two zero partials.
// vif_final: a wave per image, sixteen waves per block: adds the image's partials of all scales in double in a fixed order, writes the
//   score and, when asked, the table [2][N]: 1 / ((den + EPS) ln 10) and V / ((den + EPS) ln 10) (times 1 / N when averaging), so the
//   backward reads nothing on the host.  For the batch mean one block walks the images sixteen at a time and adds the waves' sums in
//   a fixed order: no second launch.
// vif_scale_bwd: a block takes a 16 x 32 tile of the scale's image.  It stages the tile plus 2 (K_s - 1), recomputes the five filtered
//   maps on the tile plus K_s - 1, forms there the cotangent maps of mx, W*xx, W*xr, W*rr, mr (zero beyond the stat map and in the
//   pinned branches) times the table's factor times the upstream gradient, gathers them with the transposed window (the same taps:
//   the window is even), dx_q = G(c_mx) + 2 x_q G(c_xx) + r_q G(c_xr) and the mirror image for r, and adds the adjoint of the next
//   scale's filter-and-decimate, sum_i w_{s+1}(q - 2 i) d_{s+1}[i] per axis.  Scale 0 multiplies by 255 / (hi - lo).  A null dx or dr
//   skips that side's gathers, adjoint and store.
//
// Exactness.  The file is compiled without contraction; the filter passes use explicit fmaf.  Every sum runs in a fixed order; nothing
// is allocated.  The upstream gradient enters as one factor of the two table entries, so halving it halves the gradients bit for
// bit; either side's gradient runs through the same instructions whether or not the other is asked for.  A position with srr < EPS
// adds exactly 0 to both sums and has exactly zero cotangents.  V(x, r) is NOT V(r, x).
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int VI_SCALES = 4, VI_MAX_K = 17;
constexpr int VI_MIN_SIDE = 41;                      // one position of the coarsest scale sees 41 x 41 pixels
constexpr int VI_LEAD = 3, VI_TAPS = 24;             // tap m of K sits at VI_LEAD + m; zeros before and after
constexpr int VI_TY = 16, VI_TX = 64;                // the tile of vif_scale_fwd
constexpr int VI_SR = VI_TY + VI_MAX_K - 1;          // vif_scale_fwd: rows of the staged images and of the row-pass planes
constexpr int VI_SS = VI_TX + VI_MAX_K - 1;          // vif_scale_fwd: row stride of the staged images: the tile, the halo = the aligned over-read
constexpr int VI_DS = VI_TX / 2;                     // vif_scale_fwd: row stride of the decimation's row-pass planes
constexpr int VJ_TY = 16, VJ_TX = 32;                // the tile of vif_scale_bwd
constexpr int VJ_PH = VJ_TY + VI_MAX_K - 1;          // vif_scale_bwd: rows of the cotangent maps
constexpr int VJ_SR = VJ_PH + VI_MAX_K - 1;          // vif_scale_bwd: rows of the staged images and of the row-pass planes (48: PH is a multiple of 4 at K = 17)
constexpr int VJ_SS = VJ_TX + 2 * VI_MAX_K - 2;      // vif_scale_bwd: row stride of the staged images
constexpr int VJ_PS = VJ_TX + VI_MAX_K - 1;          // vif_scale_bwd: row stride of the row-pass planes
constexpr int VJ_CS = VJ_TX + VI_MAX_K - 1;          // vif_scale_bwd: row stride of the cotangent maps: the tile, the halo = the aligned over-read
constexpr int VJ_STP = VJ_SR * VJ_SS, VJ_PLP = VJ_SR * VJ_PS, VJ_CTP = VJ_PH * VJ_CS;
constexpr size_t VJ_LDS = sizeof(float) * (2 * VJ_STP + 5 * VJ_PLP + 5 * VJ_CTP);
constexpr float VI_EPS = 1e-8f;
constexpr float VI_INV_LN10 = 0.43429448190325182765f;

static_assert(VI_SS % 4 == 0 && VJ_SS % 4 == 0 && VJ_PS % 4 == 0 && VJ_CS % 4 == 0 && VJ_PH % 4 == 0, "sixteen-byte rows");
static_assert(VI_LEAD >= 3 && VI_LEAD + VI_MAX_K + 3 <= VI_TAPS, "a strip of four outputs indexes taps VI_LEAD - 3 .. VI_LEAD + K + 2");
static_assert(2 * (VJ_TY / 2 + (VI_MAX_K - 1) / 4 + 1) * (VJ_TX / 2 + (VI_MAX_K - 1) / 4 + 1 + VJ_TX) <= 5 * VJ_CTP, "the adjoint's buffers fit the cotangent maps");

struct ViTaps { float t[VI_TAPS]; int K; };
struct ViArgs {
    ViTaps a, b;                                     // this scale's window; the next scale's (K = 0 at the last scale)
    float lo, sc, sn;                                // u = (t - lo) * sc (scale 0; lo = 0, sc = 1 below it); sigma_n_sq
};

// rows x SS mapped samples from (gy0, gx0) of the h x w plane p, 0 beyond it: every column of the stride is written, so an aligned
// over-read multiplies finite values by its zero taps
template <int SS>
__device__ __forceinline__ void vi_stage(const float* __restrict__ p, int h, int w, int gy0, int gx0, int rows, float lo, float sc,
                                         float* __restrict__ st) {
    for (int i = threadIdx.x; i < rows * SS; i += 256) {
        const int r = i / SS, c = i - r * SS;
        const int gy = gy0 + r, gx = gx0 + c;
        st[i] = ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) ? (p[(long)gy * w + gx] - lo) * sc : 0.f;
    }
}

// The statistics' row pass: `rows` rows of `strips` strips of four outputs of the five maps x, xx, xr, rr, r; output column 4 q + j of row
// r of map m into dst[m * DP + r * DS + 4 q + j], its support starting at column 4 q + j of the staged rows.
template <int SS, int DS, int DP>
__device__ __forceinline__ void vi_rows5(const float* __restrict__ sx, const float* __restrict__ sr, float* __restrict__ dst, int rows, int strips,
                                         const ViTaps& T) {
    const int nk4 = (T.K + 6) >> 2;
    for (int it = threadIdx.x; it < rows * strips; it += 256) {
        const int r = it / strips, q = it - r * strips;
        const float* __restrict__ px = sx + r * SS + 4 * q;
        const float* __restrict__ pr = sr + r * SS + 4 * q;
        float o0[4] = {0.f, 0.f, 0.f, 0.f}, o1[4] = {0.f, 0.f, 0.f, 0.f}, o2[4] = {0.f, 0.f, 0.f, 0.f}, o3[4] = {0.f, 0.f, 0.f, 0.f},
              o4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int k4 = 0; k4 < nk4; ++k4) {
            const float4 vx = *reinterpret_cast<const float4*>(px + 4 * k4);
            const float4 vr = *reinterpret_cast<const float4*>(pr + 4 * k4);
            const float ax[4] = {vx.x, vx.y, vx.z, vx.w}, ar[4] = {vr.x, vr.y, vr.z, vr.w};
            const int t0 = VI_LEAD + 4 * k4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xx = ax[c] * ax[c], xr = ax[c] * ar[c], rr = ar[c] * ar[c];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float w = T.t[t0 + c - j];
                    o0[j] = fmaf(ax[c], w, o0[j]);
                    o1[j] = fmaf(xx, w, o1[j]);
                    o2[j] = fmaf(xr, w, o2[j]);
                    o3[j] = fmaf(rr, w, o3[j]);
                    o4[j] = fmaf(ar[c], w, o4[j]);
                }
            }
        }
        float* __restrict__ o = dst + r * DS + 4 * q;
        *reinterpret_cast<float4*>(o) = make_float4(o0[0], o0[1], o0[2], o0[3]);
        *reinterpret_cast<float4*>(o + DP) = make_float4(o1[0], o1[1], o1[2], o1[3]);
        *reinterpret_cast<float4*>(o + 2 * DP) = make_float4(o2[0], o2[1], o2[2], o2[3]);
        *reinterpret_cast<float4*>(o + 3 * DP) = make_float4(o3[0], o3[1], o3[2], o3[3]);
        *reinterpret_cast<float4*>(o + 4 * DP) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    }
}

// The gather's row pass on one map: output column 4 q + j of row r into dst[r * DS + 4 q + j]
template <int SS, int DS>
__device__ __forceinline__ void vi_rows1(const float* __restrict__ src, float* __restrict__ dst, int rows, int strips, const ViTaps& T) {
    const int nk4 = (T.K + 6) >> 2;
    for (int it = threadIdx.x; it < rows * strips; it += 256) {
        const int r = it / strips, q = it - r * strips;
        const float* __restrict__ p = src + r * SS + 4 * q;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int k4 = 0; k4 < nk4; ++k4) {
            const float4 v = *reinterpret_cast<const float4*>(p + 4 * k4);
            const float a[4] = {v.x, v.y, v.z, v.w};
            const int t0 = VI_LEAD + 4 * k4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(a[c], T.t[t0 + c - j], o[j]);
            }
        }
        *reinterpret_cast<float4*>(dst + r * DS + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// The column pass: NS outputs of column `col` of NM planes, output j's support starting at row row0 + j.  Reads rows row0 .. row0 + K + NS - 2,
// every one of which must hold finite values.
template <int NS, int NM, int DS, int DP>
__device__ __forceinline__ void vi_cols(const float* __restrict__ pl, int row0, int col, const ViTaps& T, float (&o)[NM][NS]) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
#pragma unroll
        for (int j = 0; j < NS; ++j) o[m][j] = 0.f;
    }
    const int nk = T.K - 1 + NS;
    const float* __restrict__ p = pl + row0 * DS + col;
#pragma unroll 2
    for (int k = 0; k < nk; ++k) {
        float v[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) v[m] = p[m * DP + k * DS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const float w = T.t[VI_LEAD + k - j];
#pragma unroll
            for (int m = 0; m < NM; ++m) o[m][j] = fmaf(v[m], w, o[m][j]);
        }
    }
}

// One position: the natural logarithms ln(1 + g^2 srr / (sv + sn)) and ln(1 + srr / sn), and with GRAD the cotangents of
// (mx, W*xx, W*xr, W*rr, mr) for fN d ln(1 + tn) - fD d ln(1 + td).  A `where` passes the cotangent of the branch it took, relu'(0) = 0,
// and a value pinned by a clamp passes none.
template <bool GRAD>
__device__ __forceinline__ void vi_point(float mx, float exx, float exr, float err, float mr, float sn, float fN, float fD, float& ln_num,
                                         float& ln_den, float (&c)[5]) {
    const float vx = exx - mx * mx, vr = err - mr * mr;
    const float sxx = vx > 0.f ? vx : 0.f, srr0 = vr > 0.f ? vr : 0.f;
    const float sxr = exr - mx * mr;
    const float se = srr0 + VI_EPS;
    const float g0 = sxr / se;
    float g = g0, sv = sxx - g0 * sxr, srr = srr0;
    int svm = 0;                                     // sv is 0: sxx - g0 sxr, 1: sxx, 2: a constant
    bool gl = true, sl = true;                       // g is g0; srr is srr0
    if (srr0 < VI_EPS) { g = 0.f; sv = sxx; srr = 0.f; svm = 1; gl = false; sl = false; }
    if (sxx < VI_EPS) { g = 0.f; sv = 0.f; svm = 2; gl = false; }
    if (g < 0.f) { sv = sxx; g = 0.f; svm = 1; gl = false; }
    if (sv <= VI_EPS) { sv = VI_EPS; svm = 2; }
    const float q = sv + sn;
    const float gg = g * g;
    const float tn = gg * srr / q, td = srr / sn;
    ln_num = log1pf(tn);
    ln_den = log1pf(td);
    if (GRAD) {
        const float A = fN / (1.f + tn), B = -(fD / (1.f + td));
        float srr_b = sl ? B / sn + A * (gg / q) : 0.f;
        float g0_b = gl ? A * (2.f * g * srr / q) : 0.f;
        const float sv_b = -(A * (gg * srr / (q * q)));
        float sxx_b = 0.f, sxr_b = 0.f;
        if (svm == 0) {
            sxx_b = sv_b;
            g0_b -= sv_b * sxr;
            sxr_b = -(sv_b * g0);
        } else if (svm == 1) {
            sxx_b = sv_b;
        }
        if (gl) {
            sxr_b += g0_b / se;
            srr_b -= g0_b * g0 / se;
        }
        if (!(vx > 0.f)) sxx_b = 0.f;
        if (!(vr > 0.f)) srr_b = 0.f;
        c[0] = -(2.f * mx * sxx_b) - mr * sxr_b;
        c[1] = sxx_b;
        c[2] = sxr_b;
        c[3] = srr_b;
        c[4] = -(2.f * mr * srr_b) - mx * sxr_b;
    }
}

__global__ __launch_bounds__(256) void vif_scale_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r, float* __restrict__ next_x,
                                                            float* __restrict__ next_r, float* __restrict__ part, long blocks, int h, int w, int sh,
                                                            int sw, int nh, int nw, int tiles_h, int tiles_w, const ViArgs A) {
    static_assert(VI_TX * (VI_TY / 4) == 256 && (VI_TX / 2) * (VI_TY / 2) == 256, "a strip of four rows per thread; one decimated sample per thread");
    __shared__ __attribute__((aligned(16))) float st[2 * VI_SR * VI_SS];
    __shared__ __attribute__((aligned(16))) float pl[5 * VI_SR * VI_TX];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<VI_TY, VI_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * h * w;
    const int rows = VI_TY + A.a.K - 1;
    vi_stage<VI_SS>(x + off, h, w, t.y0, t.x0, rows, A.lo, A.sc, st);
    vi_stage<VI_SS>(r + off, h, w, t.y0, t.x0, rows, A.lo, A.sc, st + VI_SR * VI_SS);
    __syncthreads();
    float num = 0.f, den = 0.f;
    if (t.y0 < sh && t.x0 < sw) {                    // block-uniform: the tile owns stat positions
        vi_rows5<VI_SS, VI_TX, VI_SR * VI_TX>(st, st + VI_SR * VI_SS, pl, rows, VI_TX / 4, A.a);
        __syncthreads();
        const int col = threadIdx.x & 63, r4 = 4 * (threadIdx.x >> 6);
        float o[5][4], unused[5];
        vi_cols<4, 5, VI_TX, VI_SR * VI_TX>(pl, r4, col, A.a, o);
        if (t.x0 + col < sw) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t.y0 + r4 + j < sh) {
                    float ln, ld;
                    vi_point<false>(o[0][j], o[1][j], o[2][j], o[3][j], o[4][j], A.sn, 0.f, 0.f, ln, ld, unused);
                    num += ln * VI_INV_LN10;
                    den += ld * VI_INV_LN10;
                }
            }
        }
    }
    block_partial_store_256(num, red, part);         // its barriers also end the column pass's reads of pl
    block_partial_store_256(den, red, part + blocks);
    if (next_x == nullptr) return;
    // the next scale: its window on the staged tile at the even positions, rows then columns
    const int Kb = A.b.K, drows = VI_TY + Kb - 1;
    for (int it = threadIdx.x; it < 2 * drows * VI_DS; it += 256) {
        const int img = it / (drows * VI_DS), rem = it - img * (drows * VI_DS);
        const int row = rem / VI_DS, j = rem - row * VI_DS;
        const float* __restrict__ s = st + img * (VI_SR * VI_SS) + row * VI_SS + 2 * j;
        float a = 0.f;
        for (int k = 0; k < Kb; ++k) a = fmaf(s[k], A.b.t[VI_LEAD + k], a);
        pl[img * (VI_SR * VI_DS) + row * VI_DS + j] = a;
    }
    __syncthreads();
    const int i = threadIdx.x / VI_DS, j = threadIdx.x - i * VI_DS;
    const int ny = t.y0 / 2 + i, nx = t.x0 / 2 + j;
    if (ny < nh && nx < nw) {
        const long noff = (long)t.plane * nh * nw + (long)ny * nw + nx;
#pragma unroll
        for (int img = 0; img < 2; ++img) {
            const float* __restrict__ p = pl + img * (VI_SR * VI_DS) + 2 * i * VI_DS + j;
            float a = 0.f;
            for (int k = 0; k < Kb; ++k) a = fmaf(p[k * VI_DS], A.b.t[VI_LEAD + k], a);
            (img ? next_r : next_x)[noff] = a;
        }
    }
}

// where scale s's partials start in the workspace (num, then den, `blocks` of each) and how many an image has
struct ViParts { long off[VI_SCALES], per_image[VI_SCALES]; };

// a wave per image, sixteen at a time; the batch mean (grid of one block) adds the sixteen waves' sums in wave order
__global__ __launch_bounds__(1024) void vif_final_kernel(const float* __restrict__ part, const ViParts P, int N, int average,
                                                         float* __restrict__ out_image, float* __restrict__ out_mean, float* __restrict__ table) {
    __shared__ double wsum[16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (long n = (long)blockIdx.x * 16 + wave; n < N; n += (long)gridDim.x * 16) {
        double num = 0.0, den = 0.0;
        for (int s = 0; s < VI_SCALES; ++s) {
            const long per = P.per_image[s], blocks = per * N;
            const float* __restrict__ p = part + P.off[s] + n * per;
            double a = 0.0, b = 0.0;
            for (long i = lane; i < per; i += 64) { a += (double)p[i]; b += (double)p[blocks + i]; }
            num += wave_sum(a);
            den += wave_sum(b);
        }
        const double D = den + 1e-8, V = (num + 1e-8) / D;
        acc += V;
        if (lane == 0) {
            out_image[n] = (float)V;
            if (table != nullptr) {
                const double f = (average ? 1.0 / (double)N : 1.0) / (D * 2.302585092994045684);
                table[n] = (float)f;
                table[N + n] = (float)(V * f);
            }
        }
    }
    if (out_mean != nullptr) {
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int i = 0; i < 16; ++i) s += wsum[i];
            out_mean[0] = (float)(s / (double)N);
        }
    }
}

__global__ __launch_bounds__(256) void vif_scale_bwd_kernel(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ table,
                                                            const float* __restrict__ g, int gN, const float* __restrict__ dnext_x,
                                                            const float* __restrict__ dnext_r, float* __restrict__ dx, float* __restrict__ dr, int N,
                                                            int C, int h, int w, int sh, int sw, int nh, int nw, int tiles_h, int tiles_w,
                                                            const ViArgs A) {
    static_assert(VJ_TX * (VJ_TY / 2) == 256, "a strip of two rows per thread");
    extern __shared__ __attribute__((aligned(16))) float vi_lds[];
    __shared__ float tw[VI_TAPS];                    // the next scale's window, for the adjoint's per-lane tap
    float* __restrict__ st = vi_lds;
    float* __restrict__ pl = st + 2 * VJ_STP;
    float* __restrict__ cot = pl + 5 * VJ_PLP;
    const PlaneTile t = plane_tile<VJ_TY, VJ_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * h * w;
    const int n = t.plane / C;
    const float up = g[gN > 1 ? n : 0];
    const float fN = table[n] * up, fD = table[N + n] * up;
    const int K = A.a.K, K1 = K - 1;
    const int PH = VJ_TY + K1, PW = VJ_TX + K1, qs = (PH + 3) >> 2, srows = 4 * qs + K1;
    vi_stage<VJ_SS>(x + off, h, w, t.y0 - K1, t.x0 - K1, srows, A.lo, A.sc, st);
    vi_stage<VJ_SS>(r + off, h, w, t.y0 - K1, t.x0 - K1, srows, A.lo, A.sc, st + VJ_STP);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < VI_TAPS; ++k) tw[k] = A.b.t[k];
    }
    __syncthreads();
    // the five filtered maps on the tile plus K - 1: rows, then columns and the cotangents of every stat position there
    vi_rows5<VJ_SS, VJ_PS, VJ_PLP>(st, st + VJ_STP, pl, srows, (PW + 3) >> 2, A.a);
    __syncthreads();
    for (int it = threadIdx.x; it < qs * VJ_CS; it += 256) {
        const int rs = it / VJ_CS, c = it - rs * VJ_CS;
        float cc[4][5];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int m = 0; m < 5; ++m) cc[j][m] = 0.f;
        }
        if (c < PW) {
            float o[5][4];
            vi_cols<4, 5, VJ_PS, VJ_PLP>(pl, 4 * rs, c, A.a, o);
            const int px = t.x0 - K1 + c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int py = t.y0 - K1 + 4 * rs + j;
                if ((unsigned)py < (unsigned)sh && (unsigned)px < (unsigned)sw) {
                    float ln, ld;
                    vi_point<true>(o[0][j], o[1][j], o[2][j], o[3][j], o[4][j], A.sn, fN, fD, ln, ld, cc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * rs + j < PH) {
#pragma unroll
                for (int m = 0; m < 5; ++m) cot[m * VJ_CTP + (4 * rs + j) * VJ_CS + c] = cc[j][m];
            }
        }
    }
    __syncthreads();
    // the gather: maps 0..2 (mx, xx, xr) serve dx, maps 2..4 (xr, rr, mr) serve dr; the window is even, so the same taps
    const int m0 = dx != nullptr ? 0 : 2, m1 = dr != nullptr ? 5 : 3;
    for (int m = m0; m < m1; ++m) vi_rows1<VJ_CS, VJ_PS>(cot + m * VJ_CTP, pl + m * VJ_PLP, PH, VJ_TX / 4, A.a);
    __syncthreads();
    const int col = threadIdx.x & 31, r2 = 2 * (threadIdx.x >> 5);
    float G[5][2];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        G[m][0] = G[m][1] = 0.f;
        if (m >= m0 && m < m1) {
            float o[1][2];
            vi_cols<2, 1, VJ_PS, VJ_PLP>(pl + m * VJ_PLP, r2, col, A.a, o);
            G[m][0] = o[0][0];
            G[m][1] = o[0][1];
        }
    }
    float ax[2], ar[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float xq = st[(r2 + j + K1) * VJ_SS + col + K1], rq = st[VJ_STP + (r2 + j + K1) * VJ_SS + col + K1];
        ax[j] = (G[0][j] + (2.f * xq) * G[1][j]) + rq * G[2][j];
        ar[j] = (G[4][j] + (2.f * rq) * G[3][j]) + xq * G[2][j];
    }
    // the adjoint of the next scale's filter-and-decimate: the cotangent maps are dead, their space holds the staged gradient and the row pass
    const int Kb = A.b.K;
    if (Kb > 0) {
        const int hb = (Kb - 1) >> 1, NI = VJ_TY / 2 + hb, NJ = VJ_TX / 2 + hb;
        const int i0 = (t.y0 - Kb + 1) / 2, j0 = (t.x0 - Kb + 1) / 2;      // both numerators are even: exact, may be negative
        const long noff = (long)t.plane * nh * nw;
        float* __restrict__ buf = cot;
        float* __restrict__ tmp = cot + NI * NJ;
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const float* __restrict__ dn = side ? dnext_r : dnext_x;
            if ((side ? dr : dx) == nullptr || dn == nullptr) continue;
            for (int it = threadIdx.x; it < NI * NJ; it += 256) {
                const int i = it / NJ, j = it - i * NJ;
                const int gi = i0 + i, gj = j0 + j;
                buf[it] = ((unsigned)gi < (unsigned)nh && (unsigned)gj < (unsigned)nw) ? dn[noff + (long)gi * nw + gj] : 0.f;
            }
            __syncthreads();
            for (int it = threadIdx.x; it < NI * VJ_TX; it += 256) {
                const int i = it / VJ_TX, qx = it - i * VJ_TX;
                float a = 0.f;
                for (int j = (qx + 1) >> 1; j <= (qx + Kb - 1) >> 1; ++j) a = fmaf(buf[i * NJ + j], tw[VI_LEAD + qx + Kb - 1 - 2 * j], a);
                tmp[it] = a;
            }
            __syncthreads();
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int qy = r2 + jj;
                float a = 0.f;
                for (int i = (qy + 1) >> 1; i <= (qy + Kb - 1) >> 1; ++i) a = fmaf(tmp[i * VJ_TX + col], tw[VI_LEAD + qy + Kb - 1 - 2 * i], a);
                if (side) ar[jj] += a; else ax[jj] += a;
            }
            __syncthreads();
        }
    }
    const int gx = t.x0 + col;
    if (gx < w) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = t.y0 + r2 + j;
            if (gy < h) {
                if (dx != nullptr) dx[off + (long)gy * w + gx] = A.sc * ax[j];
                if (dr != nullptr) dr[off + (long)gy * w + gx] = A.sc * ar[j];
            }
        }
    }
}

// the sides of the four scales' images
struct ViDims { int h[VI_SCALES], w[VI_SCALES]; };

static int vi_window(int s) { return (1 << (4 - s)) + 1; }

static int vi_dims(const char* what, long N, long C, int H, int W, ViDims* D) {
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL || N * C > 0x7fffffffL)
        return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld images of %ld channels of %d x %d)", what, N, C, H, W);
    if (H < VI_MIN_SIDE || W < VI_MIN_SIDE) return fail(FAOCTASR_EINVAL, "%s: sides %d x %d below %d", what, H, W, VI_MIN_SIDE);
    if ((long)H * W > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: a plane of %d x %d exceeds 2^31 - 1 samples", what, H, W);
    D->h[0] = H;
    D->w[0] = W;
    for (int s = 1; s < VI_SCALES; ++s) {
        D->h[s] = (D->h[s - 1] - vi_window(s) + 2) / 2;
        D->w[s] = (D->w[s - 1] - vi_window(s) + 2) / 2;
    }
    return FAOCTASR_OK;
}

static int vi_scale_ok(const char* what, int scale) {
    if (scale < 0 || scale >= VI_SCALES) return fail(FAOCTASR_EINVAL, "%s: scale %d (0..%d)", what, scale, VI_SCALES - 1);
    return FAOCTASR_OK;
}

// the grid of vif_scale_fwd at scale s: the filtered map of the next scale's window, or at the last scale the stat map
static int vi_fwd_tiles(const char* what, long planes, const ViDims& D, int s, int* tiles_h, int* tiles_w, long* blocks) {
    const int Kg = s + 1 < VI_SCALES ? vi_window(s + 1) : vi_window(s);
    if (plane_tiles(planes, D.h[s] - Kg + 1, D.w[s] - Kg + 1, VI_TY, VI_TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

static void vi_taps(int K, ViTaps* T) {
    *T = ViTaps{};
    T->K = K;
    if (K == 0) return;
    double v[VI_MAX_K], sum = 0.0;
    const double sd = K / 5.0;
    for (int k = 0; k < K; ++k) { const double d = k - (K - 1) / 2.0; v[k] = exp(-(d * d) / (2.0 * sd * sd)); sum += v[k]; }
    for (int k = 0; k < K; ++k) T->t[VI_LEAD + k] = (float)(v[k] / sum);
}

static int vi_args(const char* what, int scale, float lo, float hi, float sn, ViArgs* A) {
    if (!(hi > lo) || !(hi - lo < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: value_range (%g, %g) must be finite with hi > lo", what, (double)lo, (double)hi);
    if (!(sn > 0.f) || !(sn < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: sigma_n_sq %g must be positive and finite", what, (double)sn);
    vi_taps(vi_window(scale), &A->a);
    vi_taps(scale + 1 < VI_SCALES ? vi_window(scale + 1) : 0, &A->b);
    A->lo = scale == 0 ? lo : 0.f;
    A->sc = scale == 0 ? (float)(255.0 / ((double)hi - (double)lo)) : 1.f;
    A->sn = sn;
    return FAOCTASR_OK;
}

static int vi_parts(const char* what, long N, long C, const ViDims& D, ViParts* P, long* total) {
    long at = 0;
    for (int s = 0; s < VI_SCALES; ++s) {
        int rc, th, tw;
        long blocks;
        if ((rc = vi_fwd_tiles(what, N * C, D, s, &th, &tw, &blocks))) return rc;
        P->off[s] = at;
        P->per_image[s] = blocks / N;
        at += 2 * blocks;
    }
    *total = at;
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_vif_workspace_floats(long N, long C, int H, int W) {
    ViDims D;
    ViParts P;
    long total;
    if (vi_dims("vif_workspace_floats", N, C, H, W, &D) || vi_parts("vif_workspace_floats", N, C, D, &P, &total)) return -1;
    return total;
}

extern "C" int faoctasr_vif_scale_fwd(const float* x, const float* r, float* next_x, float* next_r, float* workspace, long N, long C, int H, int W,
                                      int scale, float lo, float hi, float sigma_n_sq, faoctasr_stream_t stream) {
    if (!x || !r || !workspace) return fail(FAOCTASR_EINVAL, "vif_scale_fwd: null pointer");
    int rc, th, tw;
    long blocks, total;
    ViDims D;
    ViParts P;
    ViArgs A;
    if ((rc = vi_scale_ok("vif_scale_fwd", scale))) return rc;
    const bool last = scale == VI_SCALES - 1;
    if (last ? (next_x || next_r) : (!next_x || !next_r))
        return fail(FAOCTASR_EINVAL, "vif_scale_fwd: every scale but the last writes both images of the next one, the last none");
    if ((rc = vi_dims("vif_scale_fwd", N, C, H, W, &D))) return rc;
    if ((rc = vi_args("vif_scale_fwd", scale, lo, hi, sigma_n_sq, &A))) return rc;
    if ((rc = vi_parts("vif_scale_fwd", N, C, D, &P, &total))) return rc;
    if ((rc = vi_fwd_tiles("vif_scale_fwd", N * C, D, scale, &th, &tw, &blocks))) return rc;
    const int h = D.h[scale], w = D.w[scale];
    hipLaunchKernelGGL(vif_scale_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, r, next_x, next_r, workspace + P.off[scale],
                       blocks, h, w, h - A.a.K + 1, w - A.a.K + 1, last ? 0 : D.h[scale + 1], last ? 0 : D.w[scale + 1], th, tw, A);
    return check_launch("vif_scale_fwd");
}

extern "C" int faoctasr_vif_final(const float* workspace, long N, long C, int H, int W, int average, float* out_image, float* out_mean, float* table,
                                  faoctasr_stream_t stream) {
    if (!workspace || !out_image) return fail(FAOCTASR_EINVAL, "vif_final: null pointer");
    int rc;
    long total;
    ViDims D;
    ViParts P;
    if ((rc = vi_dims("vif_final", N, C, H, W, &D))) return rc;
    if ((rc = vi_parts("vif_final", N, C, D, &P, &total))) return rc;
    const unsigned grid = out_mean ? 1u : (unsigned)((N + 15) / 16);
    hipLaunchKernelGGL(vif_final_kernel, dim3(grid), dim3(1024), 0, (hipStream_t)stream, workspace, P, (int)N, average, out_image, out_mean, table);
    return check_launch("vif_final");
}

extern "C" int faoctasr_vif_scale_bwd(const float* x, const float* r, const float* table, const float* g, int gN, const float* dnext_x,
                                      const float* dnext_r, float* dx, float* dr, long N, long C, int H, int W, int scale, float lo, float hi,
                                      float sigma_n_sq, faoctasr_stream_t stream) {
    if (!x || !r || !table || !g) return fail(FAOCTASR_EINVAL, "vif_scale_bwd: null pointer");
    if (!dx && !dr) return fail(FAOCTASR_EINVAL, "vif_scale_bwd: neither dx nor dr");
    if (gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "vif_scale_bwd: gN must be 1 or N");
    int rc, th, tw;
    long blocks;
    ViDims D;
    ViArgs A;
    if ((rc = vi_scale_ok("vif_scale_bwd", scale))) return rc;
    const bool last = scale == VI_SCALES - 1;
    if (last ? (dnext_x || dnext_r) : ((dx != nullptr) != (dnext_x != nullptr) || (dr != nullptr) != (dnext_r != nullptr)))
        return fail(FAOCTASR_EINVAL, "vif_scale_bwd: every scale but the last takes the next scale's gradient of each side it writes, the last none");
    if ((rc = vi_dims("vif_scale_bwd", N, C, H, W, &D))) return rc;
    if ((rc = vi_args("vif_scale_bwd", scale, lo, hi, sigma_n_sq, &A))) return rc;
    const int h = D.h[scale], w = D.w[scale];
    if (!plane_tiles(N * C, h, w, VJ_TY, VJ_TX, &th, &tw, &blocks))
        return fail(FAOCTASR_EUNSUPPORTED, "vif_scale_bwd: %ld planes of %ld tiles exceed the grid", N * C, (long)th * tw);
    lds_optin((const void*)vif_scale_bwd_kernel, VJ_LDS);
    hipLaunchKernelGGL(vif_scale_bwd_kernel, dim3((unsigned)blocks), dim3(256), VJ_LDS, (hipStream_t)stream, x, r, table, g, gN, dnext_x, dnext_r, dx, dr,
                       (int)N, (int)C, h, w, h - A.a.K + 1, w - A.a.K + 1, last ? 0 : D.h[scale + 1], last ? 0 : D.w[scale + 1], th, tw, A);
    return check_launch("vif_scale_bwd");
}
