// GMSD, the gradient magnitude similarity deviation (Xue, Zhang, Mou & Bovik 2014), and its multi-scale form MS-GMSD (Zhang, Shen,
// Wang & Li 2017), grey planes, fp32.  For a pair a, b of (N, C, H, W), channels independent grey planes pooled inside an image:
//
//   u = (x - lo) / (hi - lo), value_range = (lo, hi), hi > lo;   pool(t) = avg_pool2d(t, 2): floor pooling, an odd last row or column is dropped
//   Prewitt gradients, zero padding 1, the size of their input:
//     gx_p = (1/3) sum_{dy = -1..1} (t[y + dy][x - 1] - t[y + dy][x + 1]),  gy_p the same on the other axis,  m_p = sqrt(gx_p^2 + gy_p^2), no epsilon
//   g_p = (2 ma_p mb_p + c) / (ma_p^2 + mb_p^2 + c),  c = 0.0026 by default (170 / 255^2)
//   V[n] = the population variance of g_p over the channels and positions of image n
//   GMSD[n] = sqrt(V[n]) on the once-pooled pair pool(u_a), pool(u_b); sides at least 2
//   MS-GMSD[n] = sqrt(sum_j w_j V_j[n]), scale 1 the mapped input itself, scale j + 1 = pool(scale j); 1 <= M <= 5 weights, each finite and
//     >= 0, not all zero, default (0.096, 0.596, 0.289, 0.019); sides at least 2^(M - 1); a scale of weight 0 contributes exactly nothing
//   Both are distortions: 0 for identical images, larger is worse.  Where m_p == 0 that image's direction (gx, gy) / m is taken as (0, 0);
//   where an image's score is 0 its gradient is exactly zero.
//
// The kernels work with d_p = 1 - g_p = (ma - mb)^2 / (ma^2 + mb^2 + c), which is non-negative and free of cancellation near g = 1; the
// variance of d is the variance of g.
//
// gmsd_index<POOLED>, once per scale: a block takes a 16 x 64 tile of one plane of the scale's map, stages the tile plus a halo of 1 of
//   both images into LDS, forms both Prewitt responses of four neighbouring outputs per thread from one read of the 3 x 6 samples
//   around them (3-sums of sample differences, the vertical differences shared along the strip: gm_prewitt) and writes ONE partial
//   sum of d_p and ONE of d_p^2 per block (per-thread sum, 64-lane butterfly, the four waves in a fixed order: no atomics).  POOLED stages
//   through the affine map and the 2 x 2 mean straight from a, b (plain GMSD: the pooled pair is never stored); the other form stages a
//   scale as it is (scale 1 through the affine map) and, given a next-scale pointer, also writes the 2 x 2 means of the tile's interior
//   from the staged tile.  Both forms share one tile body.  A null workspace only pools.
// gmsd_final: one block, a wave per image: per scale of positive weight it adds the image's partials in double in a fixed order,
//   mean_d = sum d / P, V = sum d^2 / P - mean_d^2 clamped at 0, S = sqrt(sum_j w_j V_j); writes the scores, their mean and, when asked,
//   the table [2][M][N]: mean_d and coef = w_j / (S[n] P_j) (times 1 / N when averaging; 0 where S[n] == 0), so the backward reads
//   nothing on the host.
// gmsd_grad<POOLED>, once per scale, coarsest first: a block takes a 16 x 32 tile, recomputes the magnitudes on the tile plus 1 from a
//   staged halo of 2, forms there k_p = coef g_up (mean_d - d_p) and the cotangent maps k_p dg/dma (gx, gy) / ma (zero beyond the map),
//   gathers them with the transposed Prewitt stencil and in the same epilogue adds the adjoint of the pooling between scales,
//   0.25 d_coarse[y >> 1][x >> 1], spreads 2 x 2 to full resolution in the pooled form, and applies the 1 / (hi - lo) of the map.  A null
//   da / db skips that side's maps, gathers and stores; an image whose coef is 0 skips its own term altogether.
//
// Exactness.  The file is compiled without contraction; what mixes the two images goes through gm_sim / gm_dsim, which are symmetric
// in the two sides: swapping a and b leaves the score bit for bit and swaps the gradients; for a == b every d_p is exactly 0, the score 0
// and both gradients exactly 0.  The upstream gradient enters as one factor of k_p, so halving it halves the gradients.  Both forms
// form the 2 x 2 mean in one order, so GMSD is MS-GMSD with weights (0, 1) bit for bit.  Every sum runs in a fixed order; nothing is
// allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int GM_MAX_SCALES = 5;
constexpr int GF_TY = 16, GF_TX = 64;                // the tile of gmsd_index
constexpr int GF_PS = 72;                            // gmsd_index: row stride of the staged images (the tile, the halo, a multiple of 4)
constexpr int GB_TY = 16, GB_TX = 32;                // the tile of gmsd_grad
constexpr int GB_QY = GB_TY + 2, GB_QX = GB_TX + 2;  // the cotangent region: the tile plus 1
constexpr int GB_PY = GB_TY + 4, GB_PS = GB_TX + 4;  // the staged region: the tile plus 2
constexpr float GM_THIRD = 1.f / 3.f;

__device__ __forceinline__ float gm_mean4(float t00, float t01, float t10, float t11) { return ((t00 + t01) + (t10 + t11)) * 0.25f; }

// One value of a scale's map at (gy, gx), 0 beyond the h x w map.  POOLED: the 2 x 2 mean of the mapped source (row stride W) at
// (2 gy, 2 gx); otherwise the mapped sample itself (W == w; deeper scales pass lo = 0, sc = 1, which changes no bit)
template <bool POOLED>
__device__ __forceinline__ float gm_load(const float* __restrict__ p, int W, int h, int w, int gy, int gx, float lo, float sc) {
    if ((unsigned)gy >= (unsigned)h || (unsigned)gx >= (unsigned)w) return 0.f;
    if (POOLED) {
        const float* q = p + (long)(2 * gy) * W + 2 * gx;
        return gm_mean4((q[0] - lo) * sc, (q[1] - lo) * sc, (q[W] - lo) * sc, (q[W + 1] - lo) * sc);
    }
    return (p[(long)gy * W + gx] - lo) * sc;
}

// Stage ROWS x COLS values of both maps from (gy0, gx0) into two arrays of row stride PS
template <bool POOLED, int ROWS, int COLS, int PS>
__device__ __forceinline__ void gm_stage(const float* __restrict__ ap, const float* __restrict__ bp, int W, int h, int w, int gy0, int gx0,
                                         float lo, float sc, float* __restrict__ sa, float* __restrict__ sb) {
    for (int i = threadIdx.x; i < ROWS * COLS; i += 256) {
        const int r = i / COLS, c = i - r * COLS;
        sa[r * PS + c] = gm_load<POOLED>(ap, W, h, w, gy0 + r, gx0 + c, lo, sc);
        sb[r * PS + c] = gm_load<POOLED>(bp, W, h, w, gy0 + r, gx0 + c, lo, sc);
    }
}

// Both Prewitt responses of NS neighbouring outputs of a row from the 3 x (NS + 2) samples around them, p at the sample above and left
// of the first output.  The 3-sums are sums of DIFFERENCES of samples, not differences of 3-sums: the mapped images carry a mean level
// (0.5 for value_range (-1, 1)) which a 3-sum would round at its own magnitude, and that rounding, divided by m_p, is what the direction
// (gx, gy) / m of a weak-gradient position would inherit; neighbouring samples differ by little, so their differences are (nearly)
// exact.  The vertical differences are shared by the three outputs above them.
template <int NS>
__device__ __forceinline__ void gm_prewitt(const float* __restrict__ p, int stride, float (&gx)[NS], float (&gy)[NS]) {
    float r0[NS + 2], r1[NS + 2], r2[NS + 2], dv[NS + 2];
#pragma unroll
    for (int k = 0; k < NS + 2; ++k) {
        r0[k] = p[k]; r1[k] = p[stride + k]; r2[k] = p[2 * stride + k];
        dv[k] = r0[k] - r2[k];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        gx[j] = (((r0[j] - r0[j + 2]) + (r1[j] - r1[j + 2])) + (r2[j] - r2[j + 2])) * GM_THIRD;
        gy[j] = ((dv[j] + dv[j + 1]) + dv[j + 2]) * GM_THIRD;
    }
}

__device__ __forceinline__ float gm_mag(float gx, float gy) { return sqrtf(gx * gx + gy * gy); }

// the one place where the two images meet: d = 1 - g = (ma - mb)^2 / r, r = ma^2 + mb^2 + c; gm_sim(a, b) == gm_sim(b, a) bit for bit
struct GmSim { float d, r; };
__device__ __forceinline__ GmSim gm_sim(float ma, float mb, float c) {
    GmSim s;
    const float e = ma - mb;
    s.r = (ma * ma + mb * mb) + c;
    s.d = (e * e) / s.r;
    return s;
}
// dg/d(own) = (2 other - 2 own g) / r with g = 1 - d, written without the cancellation: 2 ((other - own) + own d) / r
__device__ __forceinline__ float gm_dsim(float own, float other, const GmSim s) { return (2.f * ((other - own) + own * s.d)) / s.r; }

// The tile body of gmsd_index: this thread's four outputs of row r from column s4 of the staged tile; adds d and d^2 of those inside the map
__device__ __forceinline__ void gm_index_tile(const float* __restrict__ sa, const float* __restrict__ sb, int r, int s4, int gy, int gx0, int h,
                                              int w, float c, float& s1, float& s2) {
    float ax[4], ay[4], bx[4], by[4];
    gm_prewitt<4>(sa + r * GF_PS + s4, GF_PS, ax, ay);
    gm_prewitt<4>(sb + r * GF_PS + s4, GF_PS, bx, by);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (gy < h && gx0 + j < w) {
            const GmSim s = gm_sim(gm_mag(ax[j], ay[j]), gm_mag(bx[j], by[j]), c);
            s1 += s.d;
            s2 += s.d * s.d;
        }
    }
}

template <bool POOLED>
__global__ __launch_bounds__(256) void gmsd_index_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ next_a,
                                                         float* __restrict__ next_b, float* __restrict__ part, long blocks, long plane_stride,
                                                         int W, int h, int w, int tiles_h, int tiles_w, float lo, float sc, float c) {
    static_assert(GF_PS >= GF_TX + 2 && GF_PS % 4 == 0 && GF_TY * (GF_TX / 4) == 256 && (GF_TY / 2) * (GF_TX / 2) == 256, "one strip and one pooled value per thread");
    __shared__ __attribute__((aligned(16))) float st[2][(GF_TY + 2) * GF_PS];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<GF_TY, GF_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * plane_stride;
    gm_stage<POOLED, GF_TY + 2, GF_TX + 2, GF_PS>(a + off, b + off, W, h, w, t.y0 - 1, t.x0 - 1, lo, sc, st[0], st[1]);
    __syncthreads();
    if (!POOLED && next_a != nullptr) {              // the next scale: the 2 x 2 means of the tile's interior, from the staged tile
        const int i = threadIdx.x >> 5, j = threadIdx.x & 31;
        const int hn = h >> 1, wn = w >> 1;
        const int py = (t.y0 >> 1) + i, px = (t.x0 >> 1) + j;
        if (py < hn && px < wn) {
            const int at = (2 * i + 1) * GF_PS + 2 * j + 1;
            const long o = ((long)t.plane * hn + py) * wn + px;
            next_a[o] = gm_mean4(st[0][at], st[0][at + 1], st[0][at + GF_PS], st[0][at + GF_PS + 1]);
            next_b[o] = gm_mean4(st[1][at], st[1][at + 1], st[1][at + GF_PS], st[1][at + GF_PS + 1]);
        }
    }
    if (part == nullptr) return;                     // uniform: a scale of weight 0 only pools
    const int r = threadIdx.x >> 4, s4 = 4 * (threadIdx.x & 15);
    float s1 = 0.f, s2 = 0.f;
    gm_index_tile(st[0], st[1], r, s4, t.y0 + r, t.x0 + s4, h, w, c, s1, s2);
    block_partial_store_256(s1, red, part);
    block_partial_store_256(s2, red, part + blocks);
}

struct GmFinalArgs {
    long off[GM_MAX_SCALES];                         // where a scale's partials start: sums of d, then `blocks` further the sums of d^2
    long blocks[GM_MAX_SCALES];
    double count[GM_MAX_SCALES];                     // P_j = C h_j w_j
    double weight[GM_MAX_SCALES];
    int M;
};

__global__ __launch_bounds__(256) void gmsd_final_kernel(const float* __restrict__ ws, const GmFinalArgs A, int N, int average,
                                                         float* __restrict__ out_image, float* __restrict__ out_mean, float* __restrict__ table) {
    __shared__ double red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double total = 0.0;
    for (int n = wave; n < N; n += 4) {              // a wave per image; every lane ends with the same sums
        double acc = 0.0;
#pragma unroll 1
        for (int j = 0; j < GM_MAX_SCALES; ++j) {
            if (j < A.M) {
                double mean = 0.0;
                if (A.weight[j] > 0.0) {
                    const long per_image = A.blocks[j] / N;
                    const float* __restrict__ p1 = ws + A.off[j] + (long)n * per_image;
                    const float* __restrict__ p2 = p1 + A.blocks[j];
                    double s1 = 0.0, s2 = 0.0;
                    for (long i = lane; i < per_image; i += 64) { s1 += (double)p1[i]; s2 += (double)p2[i]; }
                    s1 = wave_sum(s1);
                    s2 = wave_sum(s2);
                    mean = s1 / A.count[j];
                    const double V = s2 / A.count[j] - mean * mean;
                    acc += A.weight[j] * (V > 0.0 ? V : 0.0);
                }
                if (table != nullptr && lane == 0) table[(long)j * N + n] = (float)mean;
            }
        }
        const double S = sqrt(acc);
        total += S;
        if (lane == 0) {
            out_image[n] = (float)S;
            if (table != nullptr) {
#pragma unroll 1
                for (int j = 0; j < GM_MAX_SCALES; ++j)
                    if (j < A.M)
                        table[(long)(A.M + j) * N + n] = S > 0.0 ? (float)(A.weight[j] / (S * A.count[j]) * (average ? 1.0 / (double)N : 1.0)) : 0.f;
            }
        }
    }
    if (lane == 0) red[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) out_mean[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)N);
}

// the transposed Prewitt stencil in gather form: cx, cy at the cotangent region's sample above and left of the output
__device__ __forceinline__ float gm_gather(const float* __restrict__ cx, const float* __restrict__ cy) {
    constexpr int Q = GB_QX;
    const float sx = ((cx[2] - cx[0]) + (cx[Q + 2] - cx[Q])) + (cx[2 * Q + 2] - cx[2 * Q]);
    const float sy = ((cy[2 * Q] - cy[0]) + (cy[2 * Q + 1] - cy[1])) + (cy[2 * Q + 2] - cy[2]);
    return (sx + sy) * GM_THIRD;
}

template <bool POOLED>
__global__ __launch_bounds__(256) void gmsd_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean_d,
                                                        const float* __restrict__ coef, const float* __restrict__ gout, int gN,
                                                        const float* __restrict__ dca, const float* __restrict__ dcb, float* __restrict__ da,
                                                        float* __restrict__ db, int C, long plane_stride, int H, int W, int h, int w,
                                                        int tiles_h, int tiles_w, float lo, float sc, float c) {
    static_assert(GB_QX % 2 == 0 && GB_TY * (GB_TX / 2) == 256, "strips of two");
    __shared__ float st[2][GB_PY * GB_PS];
    __shared__ float cot[4][GB_QY * GB_QX];          // the cotangents of gx, gy of a, then of b
    const PlaneTile t = plane_tile<GB_TY, GB_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * plane_stride;
    const int n = t.plane / C;
    const float gv = coef[n] * gout[gN > 1 ? n : 0];
    const bool own = gv != 0.f;                      // uniform: a scale of weight 0 and an image of score 0 have no term of their own
    const bool wa = da != nullptr, wb = db != nullptr;
    if (own) {
        gm_stage<POOLED, GB_PY, GB_PS, GB_PS>(a + off, b + off, W, h, w, t.y0 - 2, t.x0 - 2, lo, sc, st[0], st[1]);
        __syncthreads();
        const float md = mean_d[n];
        for (int it = threadIdx.x; it < GB_QY * (GB_QX / 2); it += 256) {
            const int r = it / (GB_QX / 2), s2 = 2 * (it - r * (GB_QX / 2));
            float ax[2], ay[2], bx[2], by[2];
            gm_prewitt<2>(st[0] + r * GB_PS + s2, GB_PS, ax, ay);
            gm_prewitt<2>(st[1] + r * GB_PS + s2, GB_PS, bx, by);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int gy = t.y0 - 1 + r, gx = t.x0 - 1 + s2 + j;
                float fa = 0.f, fb = 0.f;
                if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) {
                    const float ma = gm_mag(ax[j], ay[j]), mb = gm_mag(bx[j], by[j]);
                    const GmSim s = gm_sim(ma, mb, c);
                    const float k = gv * (md - s.d);
                    if (wa && ma > 0.f) fa = (k * gm_dsim(ma, mb, s)) / ma;
                    if (wb && mb > 0.f) fb = (k * gm_dsim(mb, ma, s)) / mb;
                }
                const int at = r * GB_QX + s2 + j;
                if (wa) { cot[0][at] = fa * ax[j]; cot[1][at] = fa * ay[j]; }
                if (wb) { cot[2][at] = fb * bx[j]; cot[3][at] = fb * by[j]; }
            }
        }
        __syncthreads();
    }
    const int r = threadIdx.x >> 4, c2 = 2 * (threadIdx.x & 15);
    const int y = t.y0 + r;
    const int hc = h >> 1, wc = w >> 1;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        float* __restrict__ out = side ? db : da;
        const float* __restrict__ dc = side ? dcb : dca;
        if (out == nullptr) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = t.x0 + c2 + j;
            if (y >= h || x >= w) continue;
            const int at = r * GB_QX + c2 + j;
            const float d = own ? gm_gather(cot[2 * side] + at, cot[2 * side + 1] + at) : 0.f;
            if (POOLED) {
                const float v = own ? sc * (0.25f * d) : 0.f;
                float* __restrict__ q = out + off + (long)(2 * y) * W + 2 * x;
                const bool ex = (W & 1) && x == w - 1, ey = (H & 1) && y == h - 1;   // the dropped column and row take no gradient
                q[0] = v; q[1] = v; q[W] = v; q[W + 1] = v;
                if (ex) { q[2] = 0.f; q[W + 2] = 0.f; }
                if (ey) { q[2 * W] = 0.f; q[2 * W + 1] = 0.f; }
                if (ex && ey) q[2 * W + 2] = 0.f;
            } else {
                float v = d;
                if (dc != nullptr) {                 // the adjoint of the pooling between scales
                    const int cy = y >> 1, cx = x >> 1;
                    const float up = (cy < hc && cx < wc) ? 0.25f * dc[((long)t.plane * hc + cy) * wc + cx] : 0.f;
                    v = own ? d + up : up;
                }
                out[off + (long)y * w + x] = sc * v;
            }
        }
    }
}

// the map of scale j: h x w
static int gm_geom(const char* what, long planes, int H, int W, int M, int j, int pooled, int* h, int* w) {
    if (M < 1 || M > GM_MAX_SCALES || j < 0 || j >= M || (pooled && M != 1))
        return fail(FAOCTASR_EINVAL, "%s: bad scale %d of %d (at most %d; the pooled form has one)", what, j, M, GM_MAX_SCALES);
    const int least = pooled ? 2 : 1 << (M - 1);
    if (planes < 1 || H < least || W < least)
        return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld planes of %d x %d; every side must be at least %d)", what, planes, H, W, least);
    if ((long)H * W > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: a plane of %d x %d exceeds 2^31 - 1 samples", what, H, W);
    *h = pooled ? H >> 1 : H >> j;
    *w = pooled ? W >> 1 : W >> j;
    return FAOCTASR_OK;
}

static int gm_tiles(const char* what, long planes, int h, int w, int TY, int TX, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, h, w, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

// where scale j's partials start in the workspace and how many blocks wrote them
static int gm_slot(const char* what, long planes, int H, int W, int M, int j, int pooled, long* off, long* blocks) {
    int rc, h, w, th, tw;
    *off = 0;
    for (int k = 0; k <= j; ++k) {
        if ((rc = gm_geom(what, planes, H, W, M, k, pooled, &h, &w))) return rc;
        if ((rc = gm_tiles(what, planes, h, w, GF_TY, GF_TX, &th, &tw, blocks))) return rc;
        if (k < j) *off += 2 * *blocks;
    }
    return FAOCTASR_OK;
}

static int gm_consts(const char* what, float lo, float hi, float c) {
    if (!(hi > lo) || !(hi - lo < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: value_range (%g, %g) must be finite with hi > lo", what, (double)lo, (double)hi);
    if (!(c > 0.f) || !(c < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: c %g must be positive and finite", what, (double)c);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_gmsd_workspace_floats(long planes, int H, int W, int scales, int pooled) {
    long off, blocks;
    if (gm_slot("gmsd_workspace_floats", planes, H, W, scales, scales - 1, pooled, &off, &blocks)) return -1;
    return off + 2 * blocks;
}

extern "C" int faoctasr_gmsd_index(const float* a, const float* b, float* next_a, float* next_b, float* workspace, long planes, int H, int W,
                                   int scales, int scale, int pooled, float lo, float hi, float c, faoctasr_stream_t stream) {
    if (!a || !b) return fail(FAOCTASR_EINVAL, "gmsd_index: null pointer");
    if ((next_a == nullptr) != (next_b == nullptr)) return fail(FAOCTASR_EINVAL, "gmsd_index: the next scale takes both images or neither");
    int rc, h, w, th, tw;
    long off, blocks;
    if ((rc = gm_geom("gmsd_index", planes, H, W, scales, scale, pooled, &h, &w))) return rc;
    if ((rc = gm_consts("gmsd_index", lo, hi, c))) return rc;
    if (pooled && (!workspace || next_a)) return fail(FAOCTASR_EINVAL, "gmsd_index: the pooled form takes a workspace and no next scale");
    if (next_a && scale == scales - 1) return fail(FAOCTASR_EINVAL, "gmsd_index: the last scale has no next scale");
    if (!workspace && !next_a) return FAOCTASR_OK;   // a last scale of weight 0: nothing to do
    if ((rc = gm_slot("gmsd_index", planes, H, W, scales, scale, pooled, &off, &blocks))) return rc;
    if ((rc = gm_tiles("gmsd_index", planes, h, w, GF_TY, GF_TX, &th, &tw, &blocks))) return rc;
    float* part = workspace ? workspace + off : nullptr;
    const float sc = (float)(1.0 / ((double)hi - (double)lo));
    if (pooled)
        hipLaunchKernelGGL(gmsd_index_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, next_a, next_b, part, blocks,
                           (long)H * W, W, h, w, th, tw, lo, sc, c);
    else
        hipLaunchKernelGGL(gmsd_index_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, next_a, next_b, part, blocks,
                           (long)h * w, w, h, w, th, tw, scale ? 0.f : lo, scale ? 1.f : sc, c);
    return check_launch("gmsd_index");
}

extern "C" int faoctasr_gmsd_final(const float* workspace, long N, long C, int H, int W, int scales, int pooled, const double* weights, int average,
                                   float* out_image, float* out_mean, float* table, faoctasr_stream_t stream) {
    if (!workspace || !weights || !out_image || !out_mean) return fail(FAOCTASR_EINVAL, "gmsd_final: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "gmsd_final: bad shape (%ld images of %ld channels)", N, C);
    GmFinalArgs A = {};
    int rc, h, w;
    double sum = 0.0;
    for (int j = 0; j < scales && j < GM_MAX_SCALES; ++j) {
        if (!(weights[j] >= 0.0) || !(weights[j] < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "gmsd_final: weight %g must be finite and >= 0", weights[j]);
        sum += weights[j];
    }
    if ((rc = gm_geom("gmsd_final", N * C, H, W, scales, 0, pooled, &h, &w))) return rc;
    if (!(sum > 0.0)) return fail(FAOCTASR_EINVAL, "gmsd_final: the weights must not all be zero");
    A.M = scales;
    for (int j = 0; j < scales; ++j) {
        if ((rc = gm_geom("gmsd_final", N * C, H, W, scales, j, pooled, &h, &w))) return rc;
        if ((rc = gm_slot("gmsd_final", N * C, H, W, scales, j, pooled, &A.off[j], &A.blocks[j]))) return rc;
        A.count[j] = (double)C * (double)h * (double)w;
        A.weight[j] = weights[j];
    }
    hipLaunchKernelGGL(gmsd_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, A, (int)N, average, out_image, out_mean, table);
    return check_launch("gmsd_final");
}

extern "C" int faoctasr_gmsd_grad(const float* a, const float* b, const float* table, const float* g, int gN, const float* dca, const float* dcb,
                                  float* da, float* db, long N, long C, int H, int W, int scales, int scale, int pooled, float lo, float hi,
                                  float c, faoctasr_stream_t stream) {
    if (!a || !b || !table || !g) return fail(FAOCTASR_EINVAL, "gmsd_grad: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "gmsd_grad: bad shape (%ld images of %ld channels)", N, C);
    if (gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "gmsd_grad: gN must be 1 or N");
    if (!da && !db) return fail(FAOCTASR_EINVAL, "gmsd_grad: neither gradient is asked for");
    if ((dca && !da) || (dcb && !db)) return fail(FAOCTASR_EINVAL, "gmsd_grad: a coarse gradient without its side");
    int rc, h, w, th, tw;
    long blocks;
    if ((rc = gm_geom("gmsd_grad", N * C, H, W, scales, scale, pooled, &h, &w))) return rc;
    if ((rc = gm_consts("gmsd_grad", lo, hi, c))) return rc;
    if ((dca || dcb) && (pooled || scale == scales - 1)) return fail(FAOCTASR_EINVAL, "gmsd_grad: the coarsest scale takes no coarse gradient");
    if ((rc = gm_tiles("gmsd_grad", N * C, h, w, GB_TY, GB_TX, &th, &tw, &blocks))) return rc;
    const float* mean_d = table + (long)scale * N;
    const float* coef = table + (long)(scales + scale) * N;
    const float sc = (float)(1.0 / ((double)hi - (double)lo));
    if (pooled)
        hipLaunchKernelGGL(gmsd_grad_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, mean_d, coef, g, gN, dca, dcb, da,
                           db, (int)C, (long)H * W, H, W, h, w, th, tw, lo, sc, c);
    else
        hipLaunchKernelGGL(gmsd_grad_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, mean_d, coef, g, gN, dca, dcb, da,
                           db, (int)C, (long)h * w, h, w, h, w, th, tw, scale ? 0.f : lo, scale ? 1.f : sc, c);
    return check_launch("gmsd_grad");
}
