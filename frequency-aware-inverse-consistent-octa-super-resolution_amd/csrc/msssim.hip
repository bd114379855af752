// Multi-scale SSIM (Wang, Simoncelli & Bovik 2003) on the window of ssim.py:7-32, fp32.  For a pair a, b of (N, C, H, W) and M
// scales, scale 1 the input and scale j + 1 = avg_pool2d(scale j, 2) (floor), with the five moments of ssim.py:17-27 at every scale
// (11-tap sigma-1.5 Gaussian, zero padding 5):
//
//   cs_p = (2 s12 + C2) / (s11 + s22 + C2)        l_p = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)
//   F_j[n] = mean_{c,h,w} cs_p (j < M),  F_M[n] = mean l_p cs_p,  MS[n] = prod_j max(F_j[n], 0)^w_j
//
// msssim_scale_fwd: a block takes a 16 x 64 tile of one plane of scale j, stages the tile plus a halo of 5 of both images into LDS,
//   runs the separable row and column pass, forms cs_p (l_p cs_p at the last scale), writes ONE partial sum per block (per-thread
//   sum, 64-lane butterfly, the four waves in a fixed order: no atomics) and, except at the last scale, the 2 x 2 means of the
//   tile's interior from the staged tile as scale j + 1 of both images.  Tile origins and sides are even, so a pooling cell
//   belongs to exactly one block.
// msssim_final: one block adds every (image, scale)'s partials in double in a fixed order, forms F_j[n], MS[n] (the powers through log and exp in double),
//   the batch mean and, when asked, the table coef[j][n] = w_j MS[n] / F_j[n] / (C h_j w_j) (0 where a factor of n is <= 0; times
//   1 / N when averaging), so the backward reads nothing on the host.
// msssim_scale_bwd: a block takes a 16 x 32 tile of scale j, recomputes the moments on a halo of 10, forms the partial-derivative
//   maps of cs (of l cs at the last scale) with respect to mu1, mu2, E[a^2] (= that of E[b^2]) and E[ab], applies the window to
//   them (symmetric: the zero-padded correlation is its own adjoint), multiplies by coef[j][n] and the upstream gradient, read
//   on the device, and in the same epilogue adds 0.25 d_coarse[y >> 1][x >> 1], the adjoint of the pooling.
//
// Exactness.  The file is compiled without contraction and every product of the two images is formed as g * (a * b), so that for
// a == b E[ab] equals E[a^2] bit for bit, cs_p == l_p == 1, MS == 1 and every partial-derivative map cancels to an exact 0;
// swapping a and b leaves every map bit for bit and swaps the gradients.  Every sum runs in a fixed order; nothing is allocated.
#include "common.h"

#pragma clang fp contract(off)

#include "ssim_window.h"

namespace faoctasr {

constexpr int MS_MAXLEV = 5;

// the five moments -> (cs, l); the same expressions in the forward and in the backward
struct MsPoint { float m1, m2, A1, B1, A2, B2; };
__device__ __forceinline__ MsPoint ms_point(const float (&m)[5], float C1, float C2) {
    MsPoint p;
    p.m1 = m[0]; p.m2 = m[1];
    const float m11 = p.m1 * p.m1, m22 = p.m2 * p.m2, m12 = p.m1 * p.m2;
    const float s11 = m[2] - m11, s22 = m[3] - m22, s12 = m[4] - m12;
    p.A1 = 2.f * m12 + C1; p.B1 = (m11 + m22) + C1;
    p.A2 = 2.f * s12 + C2; p.B2 = (s11 + s22) + C2;
    return p;
}

constexpr int MF_TY = 16, MF_TX = 64, MF_PY = MF_TY + 2 * SSIM_R, MF_PX = MF_TX + 2 * SSIM_R;     // 26 x 74 staged values per image

__global__ __launch_bounds__(256) void msssim_scale_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               float* __restrict__ pa, float* __restrict__ pb, float* __restrict__ part,
                                                               int H, int W, int tiles_h, int tiles_w, int last, float C1, float C2,
                                                               const SsimTaps tp) {
    __shared__ float as[MF_PY][MF_PX], bs[MF_PY][MF_PX];
    __shared__ float hz[5][MF_PY][MF_TX];
    __shared__ float red[4];
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const PlaneTile t = plane_tile<MF_TY, MF_TX>(tiles_h, tiles_w);
    const float* ap = a + (long)t.plane * H * W;
    const float* bp = b + (long)t.plane * H * W;
    for (int r = g; r < MF_PY; r += 4) {
        const int yy = t.y0 + r - SSIM_R;
        for (int cc = c; cc < MF_PX; cc += 64) {
            const int xx = t.x0 + cc - SSIM_R;
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            as[r][cc] = in ? ap[(long)yy * W + xx] : 0.f;
            bs[r][cc] = in ? bp[(long)yy * W + xx] : 0.f;
        }
    }
    __syncthreads();
    // the 2 x 2 means of the interior, one per thread (8 x 32 cells): floor, so a cell is written only where all four values exist
    if (pa) {
        const int py = tid >> 5, px = tid & 31;
        const int h2 = H >> 1, w2 = W >> 1;
        const int gy = (t.y0 >> 1) + py, gx = (t.x0 >> 1) + px;
        if (gy < h2 && gx < w2) {
            const int r = SSIM_R + 2 * py, q = SSIM_R + 2 * px;
            const long at = ((long)t.plane * h2 + gy) * w2 + gx;
            pa[at] = ((as[r][q] + as[r][q + 1]) + (as[r + 1][q] + as[r + 1][q + 1])) * 0.25f;
            pb[at] = ((bs[r][q] + bs[r][q + 1]) + (bs[r + 1][q] + bs[r + 1][q + 1])) * 0.25f;
        }
    }
    // row pass: thread = (column c, rows g, g + 4, ...)
    for (int r = g; r < MF_PY; r += 4) {
        float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float av = as[r][c + k], bv = bs[r][c + k], w = tp.g[k];
            s[0] += w * av; s[1] += w * bv; s[2] += w * (av * av); s[3] += w * (bv * bv); s[4] += w * (av * bv);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hz[q][r][c] = s[q];
    }
    __syncthreads();
    // column pass: thread = (column c, output rows 4 g .. 4 g + 3)
    float m[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 5; ++q) m[i][q] = 0.f;
#pragma unroll
    for (int rr = 0; rr < 14; ++rr) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hz[q][4 * g + rr][c];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (rr - i >= 0 && rr - i < 11) {
                const float w = tp.g[rr - i];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[i][q] += w * v[q];
            }
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (t.y0 + 4 * g + i < H && t.x0 + c < W) {
            const MsPoint p = ms_point(m[i], C1, C2);
            const float cs = p.A2 / p.B2;
            acc += last ? (p.A1 / p.B1) * cs : cs;
        }
    block_partial_store_256(acc, red, part);
}

struct MsFinal {
    long off[MS_MAXLEV];          // first partial of the scale
    int per_image[MS_MAXLEV];     // partials per image
    double count[MS_MAXLEV];      // C h_j w_j
    double w[MS_MAXLEV];
};

__global__ __launch_bounds__(256) void msssim_final_kernel(const float* __restrict__ ws, const MsFinal fi, int levels, int N, int average,
                                                           float* __restrict__ out_image, float* __restrict__ out_mean,
                                                           float* __restrict__ coef) {
    __shared__ double red[256];
    __shared__ double F[MS_MAXLEV], cnt[MS_MAXLEV], wt[MS_MAXLEV];
    __shared__ long off[MS_MAXLEV];
    __shared__ int per[MS_MAXLEV];
    if (threadIdx.x == 0) {                                             // static indices: the table is read where it is used
#pragma unroll
        for (int j = 0; j < MS_MAXLEV; ++j) { off[j] = fi.off[j]; per[j] = fi.per_image[j]; cnt[j] = fi.count[j]; wt[j] = fi.w[j]; }
    }
    __syncthreads();
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        for (int j = 0; j < levels; ++j) {
            // strided_sum_256 and block_tree_256 of common.h, written out: 64 images of 5 scales make 320 rounds a launch, and through
            // the helpers the kernel traced 4% slower (profiles/shared_helpers_bench.txt).  The helpers differ from this text in two
            // things, which were not measured apart: they index with long where an int does here, and every thread reads red[0]
            // before the round's last barrier where only thread 0 does here
            const int cntj = per[j];
            const float* p = ws + off[j] + (long)n * cntj;
            double s = 0.0;
            for (int i = threadIdx.x; i < cntj; i += 256) s += (double)p[i];
            red[threadIdx.x] = s;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) F[j] = red[0] / cnt[j];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            bool pos = true;
            for (int j = 0; j < levels; ++j) pos = pos && F[j] > 0.0;
            double ms = 0.0;
            if (pos) {
                double lg = 0.0;                                         // prod F_j^w_j = exp(sum w_j log F_j); exactly 1 where every F_j == 1
                for (int j = 0; j < levels; ++j) lg += wt[j] * log(F[j]);
                ms = exp(lg);
            }
            out_image[n] = (float)ms;
            total += ms;
            if (coef) {
                const double sc = average ? 1.0 / (double)N : 1.0;
                for (int j = 0; j < levels; ++j) coef[(long)j * N + n] = pos ? (float)(wt[j] * ms / F[j] / cnt[j] * sc) : 0.f;
            }
        }
    }
    if (threadIdx.x == 0) out_mean[0] = (float)(total / (double)N);
}

constexpr int MB_TY = 16, MB_TX = 32;
constexpr int MB_QY = MB_TY + 2 * SSIM_R, MB_QX = MB_TX + 2 * SSIM_R;      // region where the partial-derivative maps are needed
constexpr int MB_PY = MB_QY + 2 * SSIM_R, MB_PX = MB_QX + 2 * SSIM_R;      // input region

__global__ __launch_bounds__(256) void msssim_scale_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ coef, const float* __restrict__ gout, int gN,
                                                               const float* __restrict__ dca, const float* __restrict__ dcb,
                                                               float* __restrict__ da, float* __restrict__ db, int C, int H, int W,
                                                               int tiles_h, int tiles_w, int last, float C1, float C2, const SsimTaps tp) {
    __shared__ float as[MB_PY * MB_PX], bs[MB_PY * MB_PX];
    __shared__ float hz[5][MB_PY * MB_QX];                              // row-filtered moments; later the row-filtered maps
    __shared__ float pm[4][MB_QY * MB_QX];                              // d / d mu1, mu2, E[a^2] (= E[b^2]), E[ab]
    const PlaneTile t = plane_tile<MB_TY, MB_TX>(tiles_h, tiles_w);
    const float* ap = a + (long)t.plane * H * W;
    const float* bp = b + (long)t.plane * H * W;
    for (int i = threadIdx.x; i < MB_PY * MB_PX; i += 256) {
        const int r = i / MB_PX, c = i - r * MB_PX;
        const int yy = t.y0 + r - 2 * SSIM_R, xx = t.x0 + c - 2 * SSIM_R;
        const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        as[i] = in ? ap[(long)yy * W + xx] : 0.f;
        bs[i] = in ? bp[(long)yy * W + xx] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MB_PY * MB_QX; i += 256) {
        const int r = i / MB_QX, c = i - r * MB_QX;
        float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float av = as[r * MB_PX + c + k], bv = bs[r * MB_PX + c + k], w = tp.g[k];
            s[0] += w * av; s[1] += w * bv; s[2] += w * (av * av); s[3] += w * (bv * bv); s[4] += w * (av * bv);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hz[q][i] = s[q];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MB_QY * MB_QX; i += 256) {
        const int r = i / MB_QX, c = i - r * MB_QX;
        const int yy = t.y0 + r - SSIM_R, xx = t.x0 + c - SSIM_R;
        float f0 = 0.f, f1 = 0.f, f2 = 0.f, f4 = 0.f;
        if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float w = tp.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += w * hz[q][(r + k) * MB_QX + c];
            }
            const MsPoint p = ms_point(m, C1, C2);
            const float r2 = 1.f / p.B2, cs = p.A2 / p.B2;
            // d cs / d (mu1, mu2, e11 = e22, e12)
            const float c0 = (2.f * r2) * (cs * p.m1 - p.m2), c1 = (2.f * r2) * (cs * p.m2 - p.m1);
            if (!last) {
                f0 = c0; f1 = c1; f2 = -(cs * r2); f4 = 2.f * r2;
            } else {
                const float r1 = 1.f / p.B1, l = p.A1 / p.B1;
                const float l0 = (2.f * r1) * (p.m2 - l * p.m1), l1 = (2.f * r1) * (p.m1 - l * p.m2);
                f0 = cs * l0 + l * c0; f1 = cs * l1 + l * c1;
                f2 = -((l * cs) * r2); f4 = 2.f * (l * r2);
            }
        }
        pm[0][i] = f0; pm[1][i] = f1; pm[2][i] = f2; pm[3][i] = f4;
    }
    __syncthreads();
    // row pass over the maps: rows QY, output columns TX (reuses hz, row stride TX)
    for (int i = threadIdx.x; i < MB_QY * MB_TX; i += 256) {
        const int r = i / MB_TX, c = i - r * MB_TX;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float w = tp.g[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += w * pm[q][r * MB_QX + c + k];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) hz[q][i] = s[q];
    }
    __syncthreads();
    const int n = t.plane / C;
    const float gv = coef[n] * gout[gN > 1 ? n : 0];
    const int hc = H >> 1, wc = W >> 1;
    for (int i = threadIdx.x; i < MB_TY * MB_TX; i += 256) {
        const int r = i / MB_TX, c = i - r * MB_TX;
        const int yy = t.y0 + r, xx = t.x0 + c;
        if (yy < H && xx < W) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float w = tp.g[k];
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] += w * hz[q][(r + k) * MB_TX + c];
            }
            const float av = as[(r + 2 * SSIM_R) * MB_PX + c + 2 * SSIM_R], bv = bs[(r + 2 * SSIM_R) * MB_PX + c + 2 * SSIM_R];
            const long off = (long)t.plane * H * W + (long)yy * W + xx;
            // a dropped odd row or column receives nothing from the coarser scale
            const bool pooled = (yy >> 1) < hc && (xx >> 1) < wc;
            const long coff = ((long)t.plane * hc + (yy >> 1)) * wc + (xx >> 1);
            if (da) {
                float v = gv == 0.f ? 0.f : gv * ((s[0] + (2.f * av) * s[2]) + bv * s[3]);
                if (dca && pooled) v += 0.25f * dca[coff];
                da[off] = v;
            }
            if (db) {
                float v = gv == 0.f ? 0.f : gv * ((s[1] + (2.f * bv) * s[2]) + av * s[3]);
                if (dcb && pooled) v += 0.25f * dcb[coff];
                db[off] = v;
            }
        }
    }
}

// the shape rules of every entry point: scale `scale` (0-based) of a (planes, H, W) input has sides H >> scale, W >> scale
static int ms_shape(const char* what, long planes, int H, int W, int levels) {
    if (levels < 1 || levels > MS_MAXLEV) return fail(FAOCTASR_EUNSUPPORTED, "%s: %d scales, 1..%d are built", what, levels, MS_MAXLEV);
    if (planes < 1 || H < 1 || W < 1) return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld planes of %d x %d)", what, planes, H, W);
    if ((H >> (levels - 1)) < 1 || (W >> (levels - 1)) < 1)
        return fail(FAOCTASR_EINVAL, "%s: a %d x %d image leaves scale %d empty", what, H, W, levels);
    return FAOCTASR_OK;
}

template <int TY, int TX>
static int ms_tiles(const char* what, long planes, int h, int w, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, h, w, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

static bool ms_consts_ok(float C1, float C2) { return C1 > 0.f && C2 > 0.f && C1 < INFINITY && C2 < INFINITY; }

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_msssim_workspace_floats(long planes, int H, int W, int levels) {
    if (ms_shape("msssim_workspace_floats", planes, H, W, levels)) return -1;
    long total = 0;
    for (int j = 0; j < levels; ++j) {
        int th, tw;
        long blocks;
        if (ms_tiles<MF_TY, MF_TX>("msssim_workspace_floats", planes, H >> j, W >> j, &th, &tw, &blocks)) return -1;
        total += blocks;
    }
    return total;
}

extern "C" int faoctasr_msssim_scale_fwd(const float* a, const float* b, float* pa, float* pb, float* workspace, long planes, int H, int W,
                                         int levels, int scale, float C1, float C2, faoctasr_stream_t stream) {
    if (!a || !b || !workspace) return fail(FAOCTASR_EINVAL, "msssim_scale_fwd: null pointer");
    int rc;
    if ((rc = ms_shape("msssim_scale_fwd", planes, H, W, levels))) return rc;
    if (scale < 0 || scale >= levels) return fail(FAOCTASR_EINVAL, "msssim_scale_fwd: scale %d of %d", scale, levels);
    if (!ms_consts_ok(C1, C2)) return fail(FAOCTASR_EINVAL, "msssim_scale_fwd: the constants C1 %g, C2 %g must be positive and finite", (double)C1, (double)C2);
    const int last = scale == levels - 1;
    if (last ? (pa || pb) : (!pa || !pb))
        return fail(FAOCTASR_EINVAL, "msssim_scale_fwd: the pooled pair is written at every scale but the last, and only there");
    long off = 0, blocks = 0;
    int th = 0, tw = 0;
    for (int j = 0; j <= scale; ++j) {
        off += blocks;
        if ((rc = ms_tiles<MF_TY, MF_TX>("msssim_scale_fwd", planes, H >> j, W >> j, &th, &tw, &blocks))) return rc;
    }
    hipLaunchKernelGGL(msssim_scale_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, pa, pb, workspace + off,
                       H >> scale, W >> scale, th, tw, last, C1, C2, ssim_taps());
    return check_launch("msssim_scale_fwd");
}

extern "C" int faoctasr_msssim_final(const float* workspace, long N, long C, int H, int W, int levels, const double* weights, int average,
                                     float* out_image, float* out_mean, float* coef, faoctasr_stream_t stream) {
    if (!workspace || !weights || !out_image || !out_mean) return fail(FAOCTASR_EINVAL, "msssim_final: null pointer");
    if (N < 1 || C < 1) return fail(FAOCTASR_EINVAL, "msssim_final: bad shape (%ld images of %ld channels)", N, C);
    int rc;
    if ((rc = ms_shape("msssim_final", N * C, H, W, levels))) return rc;
    MsFinal fi;
    long off = 0;
    for (int j = 0; j < levels; ++j) {
        if (!(weights[j] > 0.0) || !(weights[j] < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "msssim_final: weight %d is %g, not positive and finite", j, weights[j]);
        int th, tw;
        long blocks;
        if ((rc = ms_tiles<MF_TY, MF_TX>("msssim_final", N * C, H >> j, W >> j, &th, &tw, &blocks))) return rc;
        fi.off[j] = off;
        fi.per_image[j] = (int)(blocks / N);
        fi.count[j] = (double)C * (double)(H >> j) * (double)(W >> j);
        fi.w[j] = weights[j];
        off += blocks;
    }
    for (int j = levels; j < MS_MAXLEV; ++j) { fi.off[j] = 0; fi.per_image[j] = 0; fi.count[j] = 1.0; fi.w[j] = 1.0; }
    hipLaunchKernelGGL(msssim_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, fi, levels, (int)N, average, out_image, out_mean, coef);
    return check_launch("msssim_final");
}

extern "C" int faoctasr_msssim_scale_bwd(const float* a, const float* b, const float* coef, const float* g, int gN, const float* dca,
                                         const float* dcb, float* da, float* db, long N, long C, int H, int W, int levels, int scale, float C1,
                                         float C2, faoctasr_stream_t stream) {
    if (!a || !b || !coef || !g) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: null pointer");
    if (N < 1 || C < 1) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: bad shape (%ld images of %ld channels)", N, C);
    if (gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: gN must be 1 or N");
    int rc;
    if ((rc = ms_shape("msssim_scale_bwd", N * C, H, W, levels))) return rc;
    if (scale < 0 || scale >= levels) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: scale %d of %d", scale, levels);
    if (!ms_consts_ok(C1, C2)) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: the constants C1 %g, C2 %g must be positive and finite", (double)C1, (double)C2);
    if (!da && !db) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: neither gradient is asked for");
    const int last = scale == levels - 1;
    if (last && (dca || dcb)) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: the last scale has no coarser gradient");
    if (!last && ((da && !dca) || (db && !dcb))) return fail(FAOCTASR_EINVAL, "msssim_scale_bwd: the coarser scale's gradient is missing");
    int th, tw;
    long blocks;
    if ((rc = ms_tiles<MB_TY, MB_TX>("msssim_scale_bwd", N * C, H >> scale, W >> scale, &th, &tw, &blocks))) return rc;
    hipLaunchKernelGGL(msssim_scale_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, coef + (long)scale * N, g, gN,
                       da ? dca : nullptr, db ? dcb : nullptr, da, db, (int)C, H >> scale, W >> scale, th, tw, last, C1, C2, ssim_taps());
    return check_launch("msssim_scale_bwd");
}
