// HaarPSI, the Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok & Wiegand 2018), grey planes, fp32.
// For a pair x, y of (N, C, H, W) with value_range (lo, hi), c and alpha:
//
//   u = (x - lo) 255 / (hi - lo);  u2[i, j] = the 2 x 2 mean of u at (2i, 2j), samples beyond the image 0, divisor 4: h = ceil(H / 2), w = ceil(W / 2)
//   g^v_k[i, j] = 2^-k sum_{q = j - K/2 + 1}^{j + K/2} (sum_{r = i - K/2 + 1}^{i} u2[r, q] - sum_{r = i + 1}^{i + K/2} u2[r, q]),  K = 2^k, k = 1, 2, 3,
//   g^h_k the same with rows and columns exchanged, u2 zero outside the map;  a_k = |g^o_k(x)|, b_k = |g^o_k(y)|
//   S_o = 1/2 sum_{k = 1, 2} (2 a_k b_k + c) / (a_k^2 + b_k^2 + c),   W_o = max(a_3, b_3)
//   r[n] = sum_{ch, o, p} sigmoid(alpha S_o) W_o / sum W_o,   HaarPSI[n] = (log(r / (1 - r)) / alpha)^2,  1 where sum W_o == 0
//
// The boxes are hierarchical: with P_1 = u2, P_2[t, l] = the 2 x 2 sum of P_1 anchored at (t, l) and P_4[t, l] = P_2[t, l] + P_2[t, l + 2] +
// P_2[t + 2, l] + P_2[t + 2, l + 2], every coefficient is four reads, m = K / 2, (t, l) = (i - m + 1, j - m + 1):
//   g^v_k = 2^-k ((P_m[t, l] + P_m[t, l + m]) - (P_m[t + m, l] + P_m[t + m, l + m])),   g^h_k = 2^-k ((P_m[t, l] + P_m[t + m, l]) - (P_m[t, l + m] + P_m[t + m, l + m])).
//
// The sums are kept in the complement of the sigmoid, where fp32 is relatively exact: with e(z) = 1 / (1 + exp(z)) = 1 - sigmoid(z),
//   num = sum (e(alpha S_o) - e(alpha)) W_o >= 0,  den = sum W_o,  q = num / den,  1 - r = e(alpha) + q,
// so that x == y gives num == 0 and r == sigmoid(alpha) without a cancellation between two rounded sums.
//
// haarpsi_index: a block takes a 16 x 64 tile of the half-resolution map of one plane, maps and subsamples the tile plus the level-3
//   halo (3 before, 4 after) of both images straight from x, y into LDS, forms P_2 and P_4 there, evaluates S_o, W_o and writes ONE partial
//   num and ONE partial den per block (per-thread sum, 64-lane butterfly, the four waves in a fixed order: no atomics).
// haarpsi_final: one block adds an image's partials in double in a fixed order, writes the scores, their mean and, when asked, the
//   table fac[0][n] = dHaarPSI/dr / den (times 1 / N when averaging), fac[1][n] = q, so the backward reads nothing on the host.
// haarpsi_grad: a block takes a 16 x 16 tile of the half-resolution map, recomputes the coefficients on the tile plus the adjoint's halo
//   (4 before, 3 after), forms the cotangents of the twelve coefficient maps of either image, applies the transposed boxes in gather
//   form down the same hierarchy (dP_4 -> dP_2 -> dP_1, four reads per level and map) and in the same epilogue the adjoint of the 2 x 2
//   mean and of the affine map: every pixel takes 0.25 * 255 / (hi - lo) * d[i >> 1][j >> 1], times fac[0][n] and the upstream gradient
//   read on the device.
//
// Exactness.  The file is compiled without contraction and every product of the two images goes through hp_sim, which is symmetric in
// its arguments: swapping x and y leaves the score bit for bit and swaps the gradients; for x == y every S is exactly 1, num exactly 0,
// the score 1 and both gradients exactly 0.  Every sum runs in a fixed order; nothing is allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

// 1 - sigmoid(z)
__device__ __forceinline__ float hp_comp(float z) { return 1.f / (1.f + expf(z)); }

// the one place where the two images meet: (2 a b + c) / (a^2 + b^2 + c) and its denominator; hp_sim(a, b) == hp_sim(b, a) bit for bit
struct HpSim { float S, D; };
__device__ __forceinline__ HpSim hp_sim(float a, float b, float c) {
    HpSim s;
    s.D = (a * a + b * b) + c;
    s.S = (2.f * (a * b) + c) / s.D;
    return s;
}
// d (1/2 S) / d a * 2 = 2 (b - a S) / D; the caller's 1/2 and this 2 cancel:  d S_o / d a_k = (b_k - a_k S_k) / D_k
__device__ __forceinline__ float hp_dsim(float a, float b, const HpSim s) { return (b - a * s.S) / s.D; }

__device__ __forceinline__ float hp_sign(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

// One value of the half-resolution map: the 2 x 2 mean of the mapped image at (2 gy, 2 gx); 0 outside the map
__device__ __forceinline__ float hp_load(const float* __restrict__ p, int H, int W, int h, int w, int gy, int gx, float lo, float sc) {
    if ((unsigned)gy >= (unsigned)h || (unsigned)gx >= (unsigned)w) return 0.f;
    const int Y = 2 * gy, X = 2 * gx;
    const bool y1 = Y + 1 < H, x1 = X + 1 < W;
    const float* q = p + (long)Y * W + X;
    const float u00 = (q[0] - lo) * sc;
    const float u01 = x1 ? (q[1] - lo) * sc : 0.f;
    const float u10 = y1 ? (q[W] - lo) * sc : 0.f;
    const float u11 = (y1 && x1) ? (q[W + 1] - lo) * sc : 0.f;
    return ((u00 + u01) + (u10 + u11)) * 0.25f;
}

// Stage PY x PX values of both half-resolution maps from (gy0, gx0) and form P_2 (valid on (PY - 1) x (PX - 1)) and P_4 (valid on
// (PY - 3) x (PX - 3)); all six arrays share the row stride PX.  Ends with a barrier.
template <int PY, int PX>
__device__ __forceinline__ void hp_stage(const float* __restrict__ xp, const float* __restrict__ yp, int H, int W, int h, int w, int gy0, int gx0,
                                         float lo, float sc, float* __restrict__ u1, float* __restrict__ v1, float* __restrict__ u2,
                                         float* __restrict__ v2, float* __restrict__ u4, float* __restrict__ v4) {
    for (int i = threadIdx.x; i < PY * PX; i += 256) {
        const int r = i / PX, c = i - r * PX;
        u1[i] = hp_load(xp, H, W, h, w, gy0 + r, gx0 + c, lo, sc);
        v1[i] = hp_load(yp, H, W, h, w, gy0 + r, gx0 + c, lo, sc);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (PY - 1) * PX; i += 256) {
        const int c = i % PX;
        if (c < PX - 1) {
            u2[i] = (u1[i] + u1[i + 1]) + (u1[i + PX] + u1[i + PX + 1]);
            v2[i] = (v1[i] + v1[i + 1]) + (v1[i + PX] + v1[i + PX + 1]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (PY - 3) * PX; i += 256) {
        const int c = i % PX;
        if (c < PX - 3) {
            u4[i] = (u2[i] + u2[i + 2]) + (u2[i + 2 * PX] + u2[i + 2 * PX + 2]);
            v4[i] = (v2[i] + v2[i + 2]) + (v2[i + 2 * PX] + v2[i + 2 * PX + 2]);
        }
    }
    __syncthreads();
}

// The six signed coefficients (v1, h1, v2, h2, v3, h3) of one image at the position whose staged index is (r + 3, c + 3)
template <int PX>
__device__ __forceinline__ void hp_coef(const float* __restrict__ p1, const float* __restrict__ p2, const float* __restrict__ p4, int r, int c,
                                        float (&g)[6]) {
    {
        const float* p = p1 + (r + 3) * PX + c + 3;
        const float A = p[0], B = p[1], C = p[PX], D = p[PX + 1];
        g[0] = 0.5f * ((A + B) - (C + D)); g[1] = 0.5f * ((A + C) - (B + D));
    }
    {
        const float* p = p2 + (r + 2) * PX + c + 2;
        const float A = p[0], B = p[2], C = p[2 * PX], D = p[2 * PX + 2];
        g[2] = 0.25f * ((A + B) - (C + D)); g[3] = 0.25f * ((A + C) - (B + D));
    }
    {
        const float* p = p4 + r * PX + c;
        const float A = p[0], B = p[4], C = p[4 * PX], D = p[4 * PX + 4];
        g[4] = 0.125f * ((A + B) - (C + D)); g[5] = 0.125f * ((A + C) - (B + D));
    }
}

constexpr int HF_TY = 16, HF_TX = 64, HF_PY = HF_TY + 7, HF_PX = HF_TX + 7;          // 23 x 71 staged values per image and level

__global__ __launch_bounds__(256) void haarpsi_index_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ part,
                                                            long blocks, int H, int W, int h, int w, int tiles_h, int tiles_w, float lo,
                                                            float sc, float c, float alpha) {
    __shared__ float lds[6][HF_PY * HF_PX];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<HF_TY, HF_TX>(tiles_h, tiles_w);
    hp_stage<HF_PY, HF_PX>(x + (long)t.plane * H * W, y + (long)t.plane * H * W, H, W, h, w, t.y0 - 3, t.x0 - 3, lo, sc, lds[0], lds[1], lds[2],
                           lds[3], lds[4], lds[5]);
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const float e0 = hp_comp(alpha);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 4 * g + i;
        if (t.y0 + r < h && t.x0 + col < w) {
            float gx[6], gy[6];
            hp_coef<HF_PX>(lds[0], lds[2], lds[4], r, col, gx);
            hp_coef<HF_PX>(lds[1], lds[3], lds[5], r, col, gy);
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const float S = 0.5f * (hp_sim(fabsf(gx[o]), fabsf(gy[o]), c).S + hp_sim(fabsf(gx[2 + o]), fabsf(gy[2 + o]), c).S);
                const float wt = fmaxf(fabsf(gx[4 + o]), fabsf(gy[4 + o]));
                num += (hp_comp(alpha * S) - e0) * wt;
                den += wt;
            }
        }
    }
    block_partial_store_256(num, red, part);
    block_partial_store_256(den, red, part + blocks);
}

__global__ __launch_bounds__(256) void haarpsi_final_kernel(const float* __restrict__ ws, long blocks, int per_image, int N, double alpha,
                                                            int average, float* __restrict__ out_image, float* __restrict__ out_mean,
                                                            float* __restrict__ fac) {
    __shared__ double red[256];
    const double e0 = 1.0 / (1.0 + exp(alpha));
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        const double num = block_tree_256(strided_sum_256(ws + (long)n * per_image, per_image), red);
        const double den = block_tree_256(strided_sum_256(ws + blocks + (long)n * per_image, per_image), red);
        if (threadIdx.x == 0) {
            double score = 1.0, f0 = 0.0, q = 0.0;
            if (den > 0.0) {
                q = num / den;
                const double om = e0 + q, r = 1.0 - om;                   // 1 - r and r
                const double L = log(r / om);
                score = (L / alpha) * (L / alpha);
                f0 = 2.0 * L / (alpha * alpha) / (r * om) / den * (average ? 1.0 / (double)N : 1.0);
            }
            out_image[n] = (float)score;
            total += score;
            if (fac) { fac[n] = (float)f0; fac[N + n] = (float)q; }
        }
    }
    if (threadIdx.x == 0) out_mean[0] = (float)(total / (double)N);
}

constexpr int HB_T = 16;                             // the tile of the half-resolution map: 32 x 32 pixels
constexpr int HB_G = HB_T + 7;                       // cotangent region: 4 before, 3 after
constexpr int HB_P = HB_T + 14;                      // staged region: the cotangent region plus 3 before, 4 after
constexpr int HB_D4 = HB_T + 3, HB_D2 = HB_T + 1;    // dP_4 at anchors -3 .. T - 1, dP_2 at -1 .. T - 1

// d[a][b] = Gp[a + m - 1][b + m - 1] + Gm[a + m - 1][b - 1] - Gm[a - 1][b + m - 1] - Gp[a - 1][b - 1] with Gp = 2^-k (G^v + G^h),
// Gm = 2^-k (G^v - G^h): the transposed four-read combination.  `at` is the cotangent-region index of (a - 1, b - 1)
template <int M>
__device__ __forceinline__ float hb_gather(const float* __restrict__ gp, const float* __restrict__ gm, int at) {
    return ((gp[at + M * HB_G + M] + gm[at + M * HB_G]) - gm[at + M]) - gp[at];
}

__global__ __launch_bounds__(256) void haarpsi_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ fac,
                                                           const float* __restrict__ gout, int gN, float* __restrict__ dx,
                                                           float* __restrict__ dy, int N, int C, int H, int W, int h, int w, int tiles_h,
                                                           int tiles_w, float lo, float sc, float c, float alpha) {
    __shared__ float pool[6][HB_P * HB_P];           // the staged maps and P_2, P_4; later dP_4 and dP_2 of both sides
    __shared__ float G[12][HB_G * HB_G];             // side s, level k: Gp at [6 s + 2 k], Gm at [6 s + 2 k + 1]
    const PlaneTile t = plane_tile<HB_T, HB_T>(tiles_h, tiles_w);
    const long plane_off = (long)t.plane * H * W;
    hp_stage<HB_P, HB_P>(x + plane_off, y + plane_off, H, W, h, w, t.y0 - 7, t.x0 - 7, lo, sc, pool[0], pool[1], pool[2], pool[3], pool[4],
                         pool[5]);
    const int n = t.plane / C;
    const float q = fac[N + n], e0 = hp_comp(alpha);
    const bool wx = dx != nullptr, wy = dy != nullptr;        // uniform: a side that is not asked for costs no cotangent, no map, no gather
    for (int i = threadIdx.x; i < HB_G * HB_G; i += 256) {
        const int r = i / HB_G, cc = i - r * HB_G;
        const int gy = t.y0 - 4 + r, gx = t.x0 - 4 + cc;
        float cx[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cy[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // cotangents of the signed coefficients
        if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) {
            float a[6], b[6];
            hp_coef<HB_P>(pool[0], pool[2], pool[4], r, cc, a);
            hp_coef<HB_P>(pool[1], pool[3], pool[5], r, cc, b);
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const float a1 = fabsf(a[o]), b1 = fabsf(b[o]), a2 = fabsf(a[2 + o]), b2 = fabsf(b[2 + o]), a3 = fabsf(a[4 + o]), b3 = fabsf(b[4 + o]);
                const HpSim s1 = hp_sim(a1, b1, c), s2 = hp_sim(a2, b2, c);
                const float S = 0.5f * (s1.S + s2.S);
                const float tc = hp_comp(alpha * S);
                const float wt = fmaxf(a3, b3);
                const float cS = (alpha * (tc * (1.f - tc))) * wt;       // d (sigmoid W) / d S
                const float cW = q - (tc - e0);                          // sigmoid - r
                if (wx) {
                    cx[o] = hp_sign(a[o]) * (cS * hp_dsim(a1, b1, s1));
                    cx[2 + o] = hp_sign(a[2 + o]) * (cS * hp_dsim(a2, b2, s2));
                    cx[4 + o] = a3 >= b3 ? hp_sign(a[4 + o]) * cW : 0.f;    // a tie goes to x
                }
                if (wy) {
                    cy[o] = hp_sign(b[o]) * (cS * hp_dsim(b1, a1, s1));
                    cy[2 + o] = hp_sign(b[2 + o]) * (cS * hp_dsim(b2, a2, s2));
                    cy[4 + o] = a3 >= b3 ? 0.f : hp_sign(b[4 + o]) * cW;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = k == 0 ? 0.5f : k == 1 ? 0.25f : 0.125f;
            if (wx) { G[2 * k][i] = f * (cx[2 * k] + cx[2 * k + 1]); G[2 * k + 1][i] = f * (cx[2 * k] - cx[2 * k + 1]); }
            if (wy) { G[6 + 2 * k][i] = f * (cy[2 * k] + cy[2 * k + 1]); G[6 + 2 * k + 1][i] = f * (cy[2 * k] - cy[2 * k + 1]); }
        }
    }
    __syncthreads();                                  // the staged maps are dead from here: pool[0..1] take dP_4, pool[2..3] dP_2
    // dP_4 at anchors (r - 3, cc - 3): (a - 1, b - 1) has the cotangent-region index (r, cc)
    for (int i = threadIdx.x; i < HB_D4 * HB_D4; i += 256) {
        const int r = i / HB_D4, cc = i - r * HB_D4;
        if (wx) pool[0][i] = hb_gather<4>(G[4], G[5], r * HB_G + cc);
        if (wy) pool[1][i] = hb_gather<4>(G[10], G[11], r * HB_G + cc);
    }
    __syncthreads();
    // dP_2 at anchors (r - 1, cc - 1): its own level, (a - 1, b - 1) at (r + 2, cc + 2), plus dP_4 at (a, b), (a, b - 2), (a - 2, b), (a - 2, b - 2)
    for (int i = threadIdx.x; i < HB_D2 * HB_D2; i += 256) {
        const int r = i / HB_D2, cc = i - r * HB_D2;
        const int at = r * HB_D4 + cc;
        if (wx) pool[2][i] = hb_gather<2>(G[2], G[3], (r + 2) * HB_G + cc + 2) +
                             ((pool[0][at + 2 * HB_D4 + 2] + pool[0][at + 2 * HB_D4]) + (pool[0][at + 2] + pool[0][at]));
        if (wy) pool[3][i] = hb_gather<2>(G[8], G[9], (r + 2) * HB_G + cc + 2) +
                             ((pool[1][at + 2 * HB_D4 + 2] + pool[1][at + 2 * HB_D4]) + (pool[1][at + 2] + pool[1][at]));
    }
    __syncthreads();
    // dP_1 of the tile, one value per thread: its own level, (a - 1, b - 1) at (r + 3, cc + 3), plus dP_2 at (a, b), (a, b - 1), (a - 1, b), (a - 1, b - 1)
    const int r = threadIdx.x >> 4, cc = threadIdx.x & 15;
    const int gy = t.y0 + r, gx = t.x0 + cc;
    if (gy < h && gx < w) {
        const float gv = fac[n] * gout[gN > 1 ? n : 0];
        const float k0 = 0.25f * sc;
        const int at = r * HB_D2 + cc;
        const int Y = 2 * gy, X = 2 * gx;
        const bool y1 = Y + 1 < H, x1 = X + 1 < W;
        const long off = plane_off + (long)Y * W + X;
        if (wx) {
            const float d = hb_gather<1>(G[0], G[1], (r + 3) * HB_G + cc + 3) +
                            ((pool[2][at + HB_D2 + 1] + pool[2][at + HB_D2]) + (pool[2][at + 1] + pool[2][at]));
            const float v = gv == 0.f ? 0.f : gv * (k0 * d);
            dx[off] = v;
            if (x1) dx[off + 1] = v;
            if (y1) dx[off + W] = v;
            if (y1 && x1) dx[off + W + 1] = v;
        }
        if (wy) {
            const float d = hb_gather<1>(G[6], G[7], (r + 3) * HB_G + cc + 3) +
                            ((pool[3][at + HB_D2 + 1] + pool[3][at + HB_D2]) + (pool[3][at + 1] + pool[3][at]));
            const float v = gv == 0.f ? 0.f : gv * (k0 * d);
            dy[off] = v;
            if (x1) dy[off + 1] = v;
            if (y1) dy[off + W] = v;
            if (y1 && x1) dy[off + W + 1] = v;
        }
    }
}

static int hp_shape(const char* what, long planes, int H, int W) {
    if (planes < 1 || H < 2 || W < 2) return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld planes of %d x %d; every side must be at least 2)", what, planes, H, W);
    return FAOCTASR_OK;
}

template <int TY, int TX>
static int hp_tiles(const char* what, long planes, int H, int W, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, (H + 1) / 2, (W + 1) / 2, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

static int hp_consts(const char* what, float lo, float hi, float c, float alpha) {
    if (!(hi > lo) || !(hi - lo < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: value_range (%g, %g) must be finite with hi > lo", what, (double)lo, (double)hi);
    if (!(c > 0.f) || !(c < INFINITY) || !(alpha > 0.f) || !(alpha < INFINITY))
        return fail(FAOCTASR_EINVAL, "%s: c %g and alpha %g must be positive and finite", what, (double)c, (double)alpha);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_haarpsi_workspace_floats(long planes, int H, int W) {
    int th, tw;
    long blocks;
    if (hp_shape("haarpsi_workspace_floats", planes, H, W)) return -1;
    if (hp_tiles<HF_TY, HF_TX>("haarpsi_workspace_floats", planes, H, W, &th, &tw, &blocks)) return -1;
    return 2 * blocks;
}

extern "C" int faoctasr_haarpsi_index(const float* x, const float* y, float* workspace, long planes, int H, int W, float lo, float hi, float c,
                                      float alpha, faoctasr_stream_t stream) {
    if (!x || !y || !workspace) return fail(FAOCTASR_EINVAL, "haarpsi_index: null pointer");
    int rc, th, tw;
    long blocks;
    if ((rc = hp_shape("haarpsi_index", planes, H, W))) return rc;
    if ((rc = hp_consts("haarpsi_index", lo, hi, c, alpha))) return rc;
    if ((rc = hp_tiles<HF_TY, HF_TX>("haarpsi_index", planes, H, W, &th, &tw, &blocks))) return rc;
    const float sc = (float)(255.0 / ((double)hi - (double)lo));
    hipLaunchKernelGGL(haarpsi_index_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, workspace, blocks, H, W, (H + 1) / 2,
                       (W + 1) / 2, th, tw, lo, sc, c, alpha);
    return check_launch("haarpsi_index");
}

extern "C" int faoctasr_haarpsi_final(const float* workspace, long N, long C, int H, int W, double alpha, int average, float* out_image,
                                      float* out_mean, float* fac, faoctasr_stream_t stream) {
    if (!workspace || !out_image || !out_mean) return fail(FAOCTASR_EINVAL, "haarpsi_final: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "haarpsi_final: bad shape (%ld images of %ld channels)", N, C);
    if (!(alpha > 0.0) || !(alpha < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "haarpsi_final: alpha %g must be positive and finite", alpha);
    int rc, th, tw;
    long blocks;
    if ((rc = hp_shape("haarpsi_final", N * C, H, W))) return rc;
    if ((rc = hp_tiles<HF_TY, HF_TX>("haarpsi_final", N * C, H, W, &th, &tw, &blocks))) return rc;
    hipLaunchKernelGGL(haarpsi_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, blocks, (int)(blocks / N), (int)N, alpha, average,
                       out_image, out_mean, fac);
    return check_launch("haarpsi_final");
}

extern "C" int faoctasr_haarpsi_grad(const float* x, const float* y, const float* fac, const float* g, int gN, float* dx, float* dy, long N,
                                     long C, int H, int W, float lo, float hi, float c, float alpha, faoctasr_stream_t stream) {
    if (!x || !y || !fac || !g) return fail(FAOCTASR_EINVAL, "haarpsi_grad: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "haarpsi_grad: bad shape (%ld images of %ld channels)", N, C);
    if (gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "haarpsi_grad: gN must be 1 or N");
    if (!dx && !dy) return fail(FAOCTASR_EINVAL, "haarpsi_grad: neither gradient is asked for");
    int rc, th, tw;
    long blocks;
    if ((rc = hp_shape("haarpsi_grad", N * C, H, W))) return rc;
    if ((rc = hp_consts("haarpsi_grad", lo, hi, c, alpha))) return rc;
    if ((rc = hp_tiles<HB_T, HB_T>("haarpsi_grad", N * C, H, W, &th, &tw, &blocks))) return rc;
    const float sc = (float)(255.0 / ((double)hi - (double)lo));
    hipLaunchKernelGGL(haarpsi_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, fac, g, gN, dx, dy, (int)N, (int)C, H, W,
                       (H + 1) / 2, (W + 1) / 2, th, tw, lo, sc, c, alpha);
    return check_launch("haarpsi_grad");
}
