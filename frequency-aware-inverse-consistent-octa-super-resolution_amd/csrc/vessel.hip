// Hessian vesselness in Frangi's form (Frangi, Niessen, Vincken & Viergever 1998), made continuous, and the continuous Dice overlap of the
// vessel maps of two images.  Grey planes, fp32.  For x of (N, C, H, W), channels independent grey planes pooled inside an image:
//
//   u = (x - lo) / (hi - lo), value_range = (lo, hi), hi > lo
//   per scale sigma: R = int(3 sigma + 0.5), t = -R..R, g = exp(-t^2 / (2 sigma^2)) / sum, g1 = -t / sigma^2 g, g2 = (t^2 / sigma^4 - 1 / sigma^2) g
//     (the sampled kernels of scipy.ndimage.gaussian_filter(order, truncate=3); nothing is renormalised after the polynomial)
//   a = sigma^2 (g2 along W, g along H) * u,  b = sigma^2 (g1, g1) * u,  d = sigma^2 (g along W, g2 along H) * u: true convolutions, zero padding,
//     the size of the input; bright == 0 (dark ridges) negates a, b, d
//   m = (a + d) / 2, h = (a - d) / 2, r = sqrt(h^2 + b^2), kappa = r - m, mu = m + r: the eigenvalues ordered by VALUE, not magnitude
//   E1 = mu^2 / (2 beta^2 kappa^2), E2 = (mu^2 + kappa^2) / (2 c^2)
//   V = exp(-E1) (1 - exp(-E2)) where kappa > 0 and E1 < 87, exactly 0 (with zero cotangents) elsewhere
//   Rsp = sum_s w_s V_s over 1..3 scales of positive weight, the weights normalised to sum 1 by the caller
//   S[n] = (2 mean(A B) + eps) / (mean(A^2) + mean(B^2) + eps),  A = Rsp(x), B = Rsp(y), means over the channels and positions of image n
//
// The host computes the taps in double, folds sigma into them (G1 = sigma g1, G2 = sigma^2 g2, so a = G2 (x) g, b = G1 (x) G1, d = g (x) G2)
// and hands them over by value in correlation order behind VS_LEAD zeros and before zeros to the end: a strip of four outputs walks its
// samples once and multiplies sample k into output j by tap[VS_LEAD + k - j], the zeros taking the places where a sample lies outside an
// output's support.  No branch, 12 FMAs per sample read.  The leading zeros also absorb the shift that lets a row strip start at a
// multiple of four floats whatever R is, so the row passes read LDS sixteen bytes at a time.
//
// vessel_index<PAIR>: a block takes a 16 x 64 tile of one plane, stages the tile plus a halo of the largest R through the affine map into
//   LDS, and per scale runs the row pass into three planes (g, G1, G2 along W) and the column pass into a, b, d in registers, four
//   outputs of a column per thread, and adds w_s V_s into the response.  PAIR then runs y through the same LDS and the same instructions
//   (one loop body, not unrolled) and writes ONE partial each of A B, A^2, B^2 per block (per-thread sum, 64-lane butterfly, the four
//   waves in a fixed order: no atomics), and, given map pointers, the two response maps the backward reads.  The other form takes one
//   image and writes its response map.  Both share one tile body.
// vessel_final: a wave per image, four images per block: adds the image's partials in double in a fixed order, writes the score, and
//   when asked the table [2][N]: S and 1 / (P D) (times 1 / N when averaging; 0 where D == 0), so the backward reads nothing on the
//   host.  A second one-block kernel adds the scores, kept in double behind the partials, to the batch mean.
// vessel_grad<DICE>: a block takes a 16 x 32 tile.  Per side it stages the image on the tile plus 2 R_max, and per scale recomputes a, b, d
//   on the tile plus R, forms there the three cotangent maps G_q w_s dV/d(a, b, d) (zero beyond the image), with G_q = 2 (other_q - S own_q) /
//   (P D) times the upstream gradient (DICE, from the two stored response maps and the table) or the upstream map at q, and gathers them
//   with the transposed filters, which are the same taps: g and G2 are even and G1 (x) G1 is even overall.  The 1 / (hi - lo) goes into the
//   epilogue.  A null dx / dy skips that side's staging, maps, gathers and stores.
//
// Exactness.  The file is compiled without contraction; the filter passes use explicit fmaf.  Both images go through the same
// instructions and meet only in products that are symmetric in the two sides, so swapping x and y leaves the score bit for bit and
// swaps the gradients; for x == y the three partials agree bit for bit, S is exactly 1 and both gradients are exactly 0.  The upstream
// gradient enters as one factor of G_q, so halving it halves the gradients.  Negating u negates a, b, d exactly.  Every sum runs in
// a fixed order; nothing is allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int VS_MAX_SCALES = 3, VS_MAX_R = 9;
constexpr int VS_LEAD = 6, VS_TAPS = 32;             // tap m of 2 R + 1 sits at VS_LEAD + m; zeros before and after
constexpr int VF_TY = 16, VF_TX = 64;                // the tile of vessel_index
constexpr int VF_SR = VF_TY + 2 * VS_MAX_R;          // vessel_index: rows of the staged image and of the row-pass planes
constexpr int VF_SS = 88;                            // vessel_index: row stride of the staged image: tile, halo, the aligned over-read
constexpr int VB_TY = 16, VB_TX = 32;                // the tile of vessel_grad
constexpr int VB_SS = 76;                            // vessel_grad: row stride of the staged image
constexpr int VB_PS = 52;                            // vessel_grad: row stride of the row-pass planes (the tile plus 2 R, in strips of four)
constexpr int VB_CS = 56;                            // vessel_grad: row stride of the cotangent maps (the tile plus 2 R, the aligned over-read)
constexpr float VS_E1_MAX = 87.f;

// one scale: t[0] = g, t[1] = sigma g1, t[2] = sigma^2 g2 in correlation order (tap m multiplies the sample at m - R), padded as above
struct VsScale { float t[3][VS_TAPS]; float w; int R; };
struct VsArgs {
    VsScale s[VS_MAX_SCALES];
    int M, Rmax;
    float lo, sc, sgn;                               // u = (x - lo) * sc; sgn = -1 for dark ridges
    float tb2, tc2, ib2, ic2;                        // 2 beta^2, 2 c^2, 1 / beta^2, 1 / c^2
};

// rows x SS mapped samples from (gy0, gx0) of the H x W plane p, 0 beyond it: every column of the stride is written, so an aligned
// over-read multiplies finite values by its zero taps
template <int SS>
__device__ __forceinline__ void vs_stage(const float* __restrict__ p, int H, int W, int gy0, int gx0, int rows, float lo, float sc,
                                         float* __restrict__ st) {
    for (int i = threadIdx.x; i < rows * SS; i += 256) {
        const int r = i / SS, c = i - r * SS;
        const int gy = gy0 + r, gx = gx0 + c;
        st[i] = ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? (p[(long)gy * W + gx] - lo) * sc : 0.f;
    }
}

// The row pass: `rows` rows of `strips` strips of four outputs, output column 4 q + j of row r into dst[kind * DP + r * DS + 4 q + j].  The
// first output's support starts at column col0 of row row0 + r of the source.  MULTI: kind i reads its own source plane src + i * SP
// (the gather: one filter per cotangent map); otherwise all three kinds read src (the Hessian: three filters of one image).
template <bool MULTI, int SS, int SP, int DS, int DP>
__device__ __forceinline__ void vs_rows(const float* __restrict__ src, int row0, int col0, float* __restrict__ dst, int rows, int strips,
                                        const VsScale& S) {
    const int ca = col0 & ~3, sh = col0 & 3;
    const int nk4 = (sh + 2 * S.R + 7) >> 2;
    const int tb = VS_LEAD - sh;                     // sample k of the aligned walk multiplies tap tb + k - j into output j
    for (int it = threadIdx.x; it < rows * strips; it += 256) {
        const int r = it / strips, q = it - r * strips;
        const float* __restrict__ p = src + (row0 + r) * SS + ca + 4 * q;
        float o0[4] = {0.f, 0.f, 0.f, 0.f}, o1[4] = {0.f, 0.f, 0.f, 0.f}, o2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int k4 = 0; k4 < nk4; ++k4) {
            const float4 v0 = *reinterpret_cast<const float4*>(p + 4 * k4);
            const float4 v1 = MULTI ? *reinterpret_cast<const float4*>(p + SP + 4 * k4) : v0;
            const float4 v2 = MULTI ? *reinterpret_cast<const float4*>(p + 2 * SP + 4 * k4) : v0;
            const float a0[4] = {v0.x, v0.y, v0.z, v0.w}, a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
            const int t0 = tb + 4 * k4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o0[j] = fmaf(a0[c], S.t[0][t0 + c - j], o0[j]);
                    o1[j] = fmaf(a1[c], S.t[1][t0 + c - j], o1[j]);
                    o2[j] = fmaf(a2[c], S.t[2][t0 + c - j], o2[j]);
                }
            }
        }
        float* __restrict__ o = dst + r * DS + 4 * q;
        *reinterpret_cast<float4*>(o) = make_float4(o0[0], o0[1], o0[2], o0[3]);
        *reinterpret_cast<float4*>(o + DP) = make_float4(o1[0], o1[1], o1[2], o1[3]);
        *reinterpret_cast<float4*>(o + 2 * DP) = make_float4(o2[0], o2[1], o2[2], o2[3]);
    }
}

// The column pass: NS outputs of column `col`, output j at row row0 + j + R of the planes: a = g along H of plane 2, b = G1 of plane 1,
// d = G2 of plane 0.  Reads rows row0 .. row0 + 2 R + NS - 1, every one of which must hold finite values.
template <int NS, int DS, int DP>
__device__ __forceinline__ void vs_cols(const float* __restrict__ pl, int row0, int col, const VsScale& S, float (&a)[NS], float (&b)[NS],
                                        float (&d)[NS]) {
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = b[j] = d[j] = 0.f;
    const int nk = 2 * S.R + NS;
    const float* __restrict__ p = pl + row0 * DS + col;
#pragma unroll 2
    for (int k = 0; k < nk; ++k) {
        const float v0 = p[k * DS], v1 = p[DP + k * DS], v2 = p[2 * DP + k * DS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            a[j] = fmaf(v2, S.t[0][VS_LEAD + k - j], a[j]);
            b[j] = fmaf(v1, S.t[1][VS_LEAD + k - j], b[j]);
            d[j] = fmaf(v0, S.t[2][VS_LEAD + k - j], d[j]);
        }
    }
}

// the vesselness of one position and, when asked, its derivatives by a, b, d
template <bool GRAD>
__device__ __forceinline__ float vs_measure(float a, float b, float d, const VsArgs& A, float& da, float& db, float& dd) {
    if (GRAD) da = db = dd = 0.f;
    const float m = 0.5f * (a + d), h = 0.5f * (a - d);
    const float r = sqrtf(h * h + b * b);
    const float kappa = r - m, mu = m + r;
    if (!(kappa > 0.f)) return 0.f;
    const float rho = mu / kappa;
    const float E1 = (rho * rho) / A.tb2;
    if (!(E1 < VS_E1_MAX)) return 0.f;
    const float E2 = (mu * mu + kappa * kappa) / A.tc2;
    const float F = expf(-E1), omq = -expm1f(-E2);
    if (GRAD) {
        const float Q = expf(-E2);
        const float ok = (omq / kappa) * A.ib2;                                   // (1 - Q) / (beta^2 kappa): bounded, E2 >= kappa^2 / (2 c^2)
        const float Vmu = F * (mu * Q * A.ic2 - ok * rho);
        const float Vka = F * (ok * (rho * rho) + Q * kappa * A.ic2);
        const float Vm = Vmu - Vka, Vr = Vmu + Vka;
        const float hr = r > 0.f ? h / r : 0.f, br = r > 0.f ? b / r : 0.f;       // the direction at an isotropic point is (0, 0)
        da = 0.5f * Vm + 0.5f * (Vr * hr);
        dd = 0.5f * Vm - 0.5f * (Vr * hr);
        db = Vr * br;
    }
    return F * omq;
}

template <bool PAIR>
__global__ __launch_bounds__(256) void vessel_index_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ map_x,
                                                           float* __restrict__ map_y, float* __restrict__ part, long blocks, int H, int W,
                                                           int tiles_h, int tiles_w, const VsArgs A) {
    static_assert(VF_TX * (VF_TY / 4) == 256 && VF_SS % 4 == 0 && VF_SS >= VF_TX - 4 + 2 * VS_MAX_R + 7, "a strip of four rows per thread");
    __shared__ __attribute__((aligned(16))) float st[VF_SR * VF_SS];
    __shared__ __attribute__((aligned(16))) float pl[3 * VF_SR * VF_TX];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<VF_TY, VF_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * H * W;
    const int col = threadIdx.x & 63, r4 = 4 * (threadIdx.x >> 6);
    const int gx = t.x0 + col, gy = t.y0 + r4;
    float first[4] = {0.f, 0.f, 0.f, 0.f}, cur[4];
#pragma unroll 1
    for (int side = 0; side < (PAIR ? 2 : 1); ++side) {
        vs_stage<VF_SS>((side ? y : x) + off, H, W, t.y0 - A.Rmax, t.x0 - A.Rmax, VF_TY + 2 * A.Rmax, A.lo, A.sc, st);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = 0.f;
#pragma unroll 1
        for (int s = 0; s < A.M; ++s) {
            const VsScale& S = A.s[s];
            vs_rows<false, VF_SS, 0, VF_TX, VF_SR * VF_TX>(st, A.Rmax - S.R, A.Rmax - S.R, pl, VF_TY + 2 * S.R, VF_TX / 4, S);
            __syncthreads();
            float a[4], b[4], d[4], u0, u1, u2;
            vs_cols<4, VF_TX, VF_SR * VF_TX>(pl, r4, col, S, a, b, d);
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] += S.w * vs_measure<false>(A.sgn * a[j], A.sgn * b[j], A.sgn * d[j], A, u0, u1, u2);
            __syncthreads();
        }
        float* __restrict__ map = side ? map_y : map_x;
        if (map != nullptr && gx < W) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (gy + j < H) map[off + (long)(gy + j) * W + gx] = cur[j];
        }
        if (PAIR && side == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) first[j] = cur[j];
        }
    }
    if (PAIR) {
        float sab = 0.f, saa = 0.f, sbb = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (gx < W && gy + j < H) {
                sab += first[j] * cur[j];
                saa += first[j] * first[j];
                sbb += cur[j] * cur[j];
            }
        }
        block_partial_store_256(sab, red, part);
        block_partial_store_256(saa, red, part + blocks);
        block_partial_store_256(sbb, red, part + 2 * blocks);
    }
}

// a wave per image; the double scores go behind the partials for vessel_mean
__global__ __launch_bounds__(256) void vessel_final_kernel(const float* __restrict__ part, long blocks, double* __restrict__ dscore, int N, double count,
                                                           double eps, int average, float* __restrict__ out_image, float* __restrict__ table) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const long per_image = blocks / N;
    const float* __restrict__ p = part + (long)n * per_image;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (long i = lane; i < per_image; i += 64) { ab += (double)p[i]; aa += (double)p[blocks + i]; bb += (double)p[2 * blocks + i]; }
    ab = wave_sum(ab);
    aa = wave_sum(aa);
    bb = wave_sum(bb);
    const double num = 2.0 * (ab / count) + eps, D = (aa / count + bb / count) + eps;
    const double S = D > 0.0 ? num / D : 1.0;        // eps == 0 and two vessel-free images
    if (lane == 0) {
        dscore[n] = S;
        out_image[n] = (float)S;
        if (table != nullptr) {
            table[n] = (float)S;
            table[N + n] = D > 0.0 ? (float)(1.0 / (count * D) * (average ? 1.0 / (double)N : 1.0)) : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void vessel_mean_kernel(const double* __restrict__ dscore, int N, float* __restrict__ out_mean) {
    __shared__ double red[256];
    const double s = block_tree_256(strided_sum_256(dscore, N), red);
    if (threadIdx.x == 0) out_mean[0] = (float)(s / (double)N);
}

constexpr int VB_SR = VB_TY + 4 * VS_MAX_R + 4;      // vessel_grad: rows of the staged image and of the row-pass planes: the halo of 2 R and the end of the column pass's last strip
constexpr int VB_PLP = VB_SR * VB_PS;                // one row-pass plane
constexpr int VB_CTP = (VB_TY + 2 * VS_MAX_R) * VB_CS;   // one cotangent map
constexpr size_t VB_LDS = sizeof(float) * (VB_SR * VB_SS + 3 * VB_PLP + 3 * VB_CTP);

template <bool DICE>
__global__ __launch_bounds__(256) void vessel_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ map_x,
                                                          const float* __restrict__ map_y, const float* __restrict__ table,
                                                          const float* __restrict__ g, int gN, float* __restrict__ dx, float* __restrict__ dy,
                                                          int N, int C, int H, int W, int tiles_h, int tiles_w, const VsArgs A) {
    static_assert(VB_TX * (VB_TY / 2) == 256 && VB_SS % 4 == 0 && VB_PS % 4 == 0 && VB_CS % 4 == 0, "a strip of two rows per thread");
    static_assert(VB_PS >= ((VB_TX + 2 * VS_MAX_R + 3) & ~3) && VB_CS >= VB_TX - 4 + 2 * VS_MAX_R + 7 && VB_SS >= VB_TX + 4 * VS_MAX_R + 6, "the over-reads stay inside a row");
    extern __shared__ __attribute__((aligned(16))) float vs_lds[];
    constexpr int CTP = VB_CTP;
    float* __restrict__ st = vs_lds;
    float* __restrict__ pl = st + VB_SR * VB_SS;
    float* __restrict__ cot = pl + 3 * VB_PLP;
    const PlaneTile t = plane_tile<VB_TY, VB_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * H * W;
    const int n = t.plane / C;
    float Sn = 0.f, f = 0.f;
    if (DICE) {
        Sn = table[n];
        f = table[N + n] * g[gN > 1 ? n : 0];
    }
    const int col = threadIdx.x & 31, r2 = 2 * (threadIdx.x >> 5);
#pragma unroll 1
    for (int side = 0; side < (DICE ? 2 : 1); ++side) {
        float* __restrict__ out = side ? dy : dx;
        if (out == nullptr) continue;
        const float* __restrict__ own = side ? map_y : map_x;
        const float* __restrict__ other = side ? map_x : map_y;
        vs_stage<VB_SS>((side ? y : x) + off, H, W, t.y0 - 2 * A.Rmax, t.x0 - 2 * A.Rmax, VB_TY + 4 * A.Rmax + 4, A.lo, A.sc, st);
        __syncthreads();
        float acc[2] = {0.f, 0.f};
#pragma unroll 1
        for (int s = 0; s < A.M; ++s) {
            const VsScale& S = A.s[s];
            const int R = S.R, qh = VB_TY + 2 * R, qw = VB_TX + 2 * R, qs = (qh + 3) >> 2;
            // a, b, d's row pass on the columns of the tile plus R, the rows of the tile plus 2 R (and up to the end of the last strip)
            vs_rows<false, VB_SS, 0, VB_PS, VB_PLP>(st, 2 * (A.Rmax - R), 2 * (A.Rmax - R), pl, 4 * qs + 2 * R, (qw + 3) >> 2, S);
            __syncthreads();
            for (int it = threadIdx.x; it < qs * VB_CS; it += 256) {
                const int rs = it / VB_CS, c = it - rs * VB_CS;
                float ca[4] = {0.f, 0.f, 0.f, 0.f}, cb[4] = {0.f, 0.f, 0.f, 0.f}, cd[4] = {0.f, 0.f, 0.f, 0.f};
                if (c < qw) {
                    float a[4], b[4], d[4];
                    vs_cols<4, VB_PS, VB_PLP>(pl, 4 * rs, c, S, a, b, d);
                    const int qx = t.x0 - R + c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int qy = t.y0 - R + 4 * rs + j;
                        if ((unsigned)qy < (unsigned)H && (unsigned)qx < (unsigned)W) {
                            const long at = off + (long)qy * W + qx;
                            const float G = DICE ? f * (2.f * (other[at] - Sn * own[at])) : g[at];
                            float da, db, dd;
                            vs_measure<true>(A.sgn * a[j], A.sgn * b[j], A.sgn * d[j], A, da, db, dd);
                            const float k = (G * S.w) * A.sgn;
                            ca[j] = k * da; cb[j] = k * db; cd[j] = k * dd;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * rs + j < qh) {                                        // plane i of the gather takes filter kind i along W
                        cot[(4 * rs + j) * VB_CS + c] = cd[j];
                        cot[CTP + (4 * rs + j) * VB_CS + c] = cb[j];
                        cot[2 * CTP + (4 * rs + j) * VB_CS + c] = ca[j];
                    }
                }
            }
            __syncthreads();
            vs_rows<true, VB_CS, CTP, VB_PS, VB_PLP>(cot, 0, 0, pl, qh, VB_TX / 4, S);
            __syncthreads();
            float a[2], b[2], d[2];
            vs_cols<2, VB_PS, VB_PLP>(pl, r2, col, S, a, b, d);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] += (a[j] + b[j]) + d[j];
            __syncthreads();
        }
        const int gx = t.x0 + col;
        if (gx < W) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (t.y0 + r2 + j < H) out[off + (long)(t.y0 + r2 + j) * W + gx] = A.sc * acc[j];
        }
    }
}

static int vs_shape(const char* what, long N, long C, int H, int W) {
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL || N * C > 0x7fffffffL || H < 1 || W < 1)
        return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld images of %ld channels of %d x %d)", what, N, C, H, W);
    if ((long)H * W > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: a plane of %d x %d exceeds 2^31 - 1 samples", what, H, W);
    return FAOCTASR_OK;
}

static int vs_tiles(const char* what, long planes, int H, int W, int TY, int TX, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, H, W, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

// the taps, in double, and every constant of the measure
static int vs_args(const char* what, const double* sigmas, const double* weights, int scales, float beta, float c, float lo, float hi, int bright,
                   VsArgs* A) {
    if (!sigmas || !weights) return fail(FAOCTASR_EINVAL, "%s: null sigmas or weights", what);
    if (scales < 1 || scales > VS_MAX_SCALES) return fail(FAOCTASR_EINVAL, "%s: %d scales (1..%d)", what, scales, VS_MAX_SCALES);
    if (!(hi > lo) || !(hi - lo < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: value_range (%g, %g) must be finite with hi > lo", what, (double)lo, (double)hi);
    if (!(beta > 0.f) || !(beta < INFINITY) || !(c > 0.f) || !(c < INFINITY))
        return fail(FAOCTASR_EINVAL, "%s: beta %g and c %g must be positive and finite", what, (double)beta, (double)c);
    *A = VsArgs{};
    A->M = scales;
    for (int s = 0; s < scales; ++s) {
        const double sg = sigmas[s];
        if (!(sg >= 0.5) || !(sg <= 3.0)) return fail(FAOCTASR_EINVAL, "%s: sigma %g outside [0.5, 3]", what, sg);
        if (!(weights[s] > 0.0) || !(weights[s] < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "%s: weight %g must be positive and finite", what, weights[s]);
        const int R = (int)(3.0 * sg + 0.5);
        double gs[2 * VS_MAX_R + 1], sum = 0.0;
        for (int i = 0; i <= 2 * R; ++i) { const double tt = i - R; gs[i] = exp(-tt * tt / (2.0 * sg * sg)); sum += gs[i]; }
        VsScale& S = A->s[s];
        for (int m = 0; m <= 2 * R; ++m) {           // correlation order: tap m is the kernel at R - m
            const double tt = R - m, gv = gs[2 * R - m] / sum;
            S.t[0][VS_LEAD + m] = (float)gv;
            S.t[1][VS_LEAD + m] = (float)(-tt / sg * gv);
            S.t[2][VS_LEAD + m] = (float)((tt * tt / (sg * sg) - 1.0) * gv);
        }
        S.w = (float)weights[s];
        S.R = R;
        if (R > A->Rmax) A->Rmax = R;
    }
    A->lo = lo;
    A->sc = (float)(1.0 / ((double)hi - (double)lo));
    A->sgn = bright ? 1.f : -1.f;
    A->tb2 = (float)(2.0 * (double)beta * (double)beta);
    A->tc2 = (float)(2.0 * (double)c * (double)c);
    A->ib2 = (float)(1.0 / ((double)beta * (double)beta));
    A->ic2 = (float)(1.0 / ((double)c * (double)c));
    return FAOCTASR_OK;
}

static long vs_even(long v) { return (v + 1) & ~1L; }

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_vessel_workspace_floats(long N, long C, int H, int W) {
    int th, tw;
    long blocks;
    if (vs_shape("vessel_workspace_floats", N, C, H, W) || vs_tiles("vessel_workspace_floats", N * C, H, W, VF_TY, VF_TX, &th, &tw, &blocks)) return -1;
    return vs_even(3 * blocks) + 2 * N;
}

extern "C" int faoctasr_vessel_index(const float* x, const float* y, float* map_x, float* map_y, float* workspace, long N, long C, int H, int W,
                                     const double* sigmas, const double* weights, int scales, float beta, float c, float lo, float hi, int bright,
                                     faoctasr_stream_t stream) {
    if (!x) return fail(FAOCTASR_EINVAL, "vessel_index: null pointer");
    if (y ? (!workspace || (map_x == nullptr) != (map_y == nullptr)) : (!map_x || map_y || workspace))
        return fail(FAOCTASR_EINVAL, "vessel_index: a pair takes a workspace and both response maps or neither; one image takes its map alone");
    int rc, th, tw;
    long blocks;
    VsArgs A;
    if ((rc = vs_shape("vessel_index", N, C, H, W))) return rc;
    if ((rc = vs_args("vessel_index", sigmas, weights, scales, beta, c, lo, hi, bright, &A))) return rc;
    if ((rc = vs_tiles("vessel_index", N * C, H, W, VF_TY, VF_TX, &th, &tw, &blocks))) return rc;
    if (y)
        hipLaunchKernelGGL(vessel_index_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, map_x, map_y, workspace, blocks, H,
                           W, th, tw, A);
    else
        hipLaunchKernelGGL(vessel_index_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, map_x, map_y, workspace, blocks, H,
                           W, th, tw, A);
    return check_launch("vessel_index");
}

extern "C" int faoctasr_vessel_final(float* workspace, long N, long C, int H, int W, double eps, int average, float* out_image, float* out_mean,
                                     float* table, faoctasr_stream_t stream) {
    if (!workspace || !out_image) return fail(FAOCTASR_EINVAL, "vessel_final: null pointer");
    if (!(eps >= 0.0) || !(eps < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "vessel_final: eps %g must be finite and >= 0", eps);
    int rc, th, tw;
    long blocks;
    if ((rc = vs_shape("vessel_final", N, C, H, W))) return rc;
    if ((rc = vs_tiles("vessel_final", N * C, H, W, VF_TY, VF_TX, &th, &tw, &blocks))) return rc;
    double* dscore = reinterpret_cast<double*>(workspace + vs_even(3 * blocks));
    if ((reinterpret_cast<uintptr_t>(dscore) & 7) != 0) return fail(FAOCTASR_EINVAL, "vessel_final: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(vessel_final_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, workspace, blocks, dscore, (int)N,
                       (double)C * (double)H * (double)W, eps, average, out_image, table);
    if ((rc = check_launch("vessel_final"))) return rc;
    if (out_mean) {
        hipLaunchKernelGGL(vessel_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dscore, (int)N, out_mean);
        rc = check_launch("vessel_final");
    }
    return rc;
}

extern "C" int faoctasr_vessel_grad(const float* x, const float* y, const float* map_x, const float* map_y, const float* table, const float* g, int gN,
                                    float* dx, float* dy, long N, long C, int H, int W, const double* sigmas, const double* weights, int scales,
                                    float beta, float c, float lo, float hi, int bright, faoctasr_stream_t stream) {
    if (!x || !g) return fail(FAOCTASR_EINVAL, "vessel_grad: null pointer");
    const bool dice = table != nullptr;
    if (dice ? (!y || !map_x || !map_y || (!dx && !dy)) : (y || map_x || map_y || dy || !dx))
        return fail(FAOCTASR_EINVAL, "vessel_grad: the index form takes both images, both response maps, the table and dx or dy; the map form x, g and dx");
    if (dice && gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "vessel_grad: gN must be 1 or N");
    int rc, th, tw;
    long blocks;
    VsArgs A;
    if ((rc = vs_shape("vessel_grad", N, C, H, W))) return rc;
    if ((rc = vs_args("vessel_grad", sigmas, weights, scales, beta, c, lo, hi, bright, &A))) return rc;
    if ((rc = vs_tiles("vessel_grad", N * C, H, W, VB_TY, VB_TX, &th, &tw, &blocks))) return rc;
    const size_t lds = VB_LDS;
    if (dice) {
        lds_optin((const void*)vessel_grad_kernel<true>, lds);
        hipLaunchKernelGGL(vessel_grad_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, y, map_x, map_y, table, g, gN, dx, dy,
                           (int)N, (int)C, H, W, th, tw, A);
    } else {
        lds_optin((const void*)vessel_grad_kernel<false>, lds);
        hipLaunchKernelGGL(vessel_grad_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, y, map_x, map_y, table, g, gN, dx, dy,
                           (int)N, (int)C, H, W, th, tw, A);
    }
    return check_launch("vessel_grad");
}
