// Soft-clDice, the centre-line Dice of Shit et al. (CVPR 2021): soft skeletons by iterated min / max pooling, and how much of each image's
// skeleton lies inside the other image.  Grey planes, fp32.  For x, y of (N, C, H, W), channels independent grey planes pooled inside an image:
//
//   u = (x - lo) / (hi - lo), value_range = (lo, hi), hi > lo; bright == 0 uses (hi - x) / (hi - lo)
//   E(I)[q] = min of I over the cross {up, left, q, right, down}, D(I)[q] = max of I over the 3 x 3 square around q, positions outside the
//     image left out at every level
//   I_0 = u, I_{k+1} = E(I_k), O_k = D(I_{k+1}), delta_k = relu(I_k - O_k), k = 0..K, K = iters in 1..10
//   s_0 = delta_0, s_k = s_{k-1} + relu(delta_k - s_{k-1} delta_k), skel(u) = s_K
//   Tprec = (sum skel(x) u_y + smooth) / (sum skel(x) + smooth), Tsens = (sum skel(y) u_x + smooth) / (sum skel(y) + smooth), the sums over
//     the channels and positions of image n; a ratio whose denominator is 0 (smooth == 0 and an empty skeleton) is taken as 0
//   S[n] = 2 Tprec Tsens / (Tprec + Tsens), 0 where the denominator is 0
//
// cldice_index<PAIR, REC>: a block takes a 16 x 64 tile of one plane and stages the tile plus a halo of K + 2 through the affine map into one
//   of two LDS planes; a position outside the image holds a quiet NaN, which fminf and fmaxf skip and which every level writes afresh, so
//   no computed value ever stands outside the image.  Level k runs the erosion from one plane into the other over the region that still
//   matters (the tile plus K + 1 - k) in strips of four along the row, sixteen bytes per LDS read, and then every thread takes its own
//   strip of four tile positions: the 3 x 3 maximum of I_{k+1} separably in registers (three rows of six values: the column maxima, then
//   the row of three), delta_k, and the update of s.  The K + 2 levels I_0..I_{K+1} take K + 1 erosions and K + 1 dilations.  PAIR then runs
//   y through the same planes and the same instructions and writes ONE partial each of sum skel(x) u_y, sum skel(x), sum skel(y) u_x,
//   sum skel(y) per block (per-thread sum, 64-lane butterfly, the four waves in a fixed order: no atomics).  REC (a gradient is needed)
//   also writes per level and position the record the backward routes by: the float c_k and one selection byte (below), and the
//   skeleton maps.  The other form takes one image and writes its skeleton map.
// cldice_final: a wave per image, four images per block: adds the image's partials in double in a fixed order, writes the score and when
//   asked the table [4][N] of dS / d(each of the four sums) (times 1 / N when averaging).  A second one-block kernel of the same call adds
//   the scores, kept in double behind the partials, to the batch mean.
// cldice_grad<DICE>: the routing kernel, a 16 x 64 tile plus a halo of K + 2.  The cotangent of skel(x) at q is G[q] = alpha u_y[q] + beta
//   (DICE: from the table times the upstream gradient) or the upstream map at q.  The reverse of the recurrence is pointwise:
//   dbar_k = G c_k with c_k = a_k prod_{j > k} b_j, a_k = [delta_k > 0] m_k (1 - s_{k-1}), b_k = 1 - m_k delta_k, m_k = [delta_k (1 - s_{k-1}) > 0],
//   a_0 = [delta_0 > 0]: the forward stored c_k, so this kernel does not depend on the forward's arithmetic.  Level by level from K down
//   to 0, in gather form: Ibar_{k+1}[p] = (what level k + 1 left at p) - sum of dbar_k[q] over the q of p's square whose arg-max is p;
//   then (what level k leaves at p) = dbar_k[p] + sum of Ibar_{k+1}[r] over the r of p's cross whose arg-min is p.  Level 0 leaves the
//   gradient by u; the direct term gamma skel(y)[q] and the sign and the division by hi - lo of the affine map go into the epilogue.  A null dx or
//   dy skips that side.
//
// Ties.  The forward does not depend on which of several equal values a minimum or maximum selects.  The selection byte names the FIRST
// position, in row-major order (cross: up, left, centre, right, down = 0..4 in bits 0-2; square: 3 (dy + 1) + (dx + 1) = 0..8 in bits 3-6),
// whose value equals the minimum or maximum, and the whole cotangent goes there: nothing is split, the total is conserved.  That is a
// valid subgradient; on plateaus it differs from the scan-order choice of a framework's pooling backward.
//
// Exactness.  The file is compiled without contraction; a product that is added uses explicit fmaf.  Minima and maxima are exact.  Both
// images go through the same instructions, so swapping x and y swaps the partials and the gradients bit for bit.  The upstream gradient
// enters as one factor of alpha, beta and gamma and everything after is linear, so halving it halves the gradients.  Every sum runs in a
// fixed order; nothing is allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int CD_MAX_ITERS = 10;
constexpr int CD_MAX_HALO = CD_MAX_ITERS + 2;
constexpr int CF_TY = 16, CF_TX = 64;                // the tile of cldice_index
constexpr int CF_SR = CF_TY + 2 * CD_MAX_HALO + 2;   // cldice_index: rows of a plane: tile, halo, one guard row above and below
constexpr int CF_SS = 96;                            // cldice_index: row stride: 4..7 guard columns (the tile starts at a multiple of four), tile, halo, guard
constexpr int CB_TY = 16, CB_TX = 64;                // the tile of cldice_grad
constexpr int CB_CELL_BYTES = 4 * 4 + 1;             // cldice_grad: four float planes and one of selection bytes over the tile plus its halo, sized per launch
constexpr unsigned char CD_NONE = 0xff;              // the selection byte of a position outside the image: matches no code

struct CdArgs {
    int K;
    float lo, range, sgn;                            // u = (x - lo) / range for sgn = 1; lo holds hi and u = (lo - x) / range for sgn = -1
};

__device__ __forceinline__ float cd_map(float v, const CdArgs& A) { return (A.sgn > 0.f ? v - A.lo : A.lo - v) / A.range; }

__device__ __forceinline__ float cd_min5(float a, float b, float c, float d, float e) { return fminf(fminf(fminf(a, b), fminf(c, d)), e); }
__device__ __forceinline__ float cd_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// four values to p[0..3], the first n of them: one 16-byte store when the caller found rows and base aligned
__device__ __forceinline__ void cd_store4(float* __restrict__ p, const float (&v)[4], int n, bool vec) {
    if (vec && n == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) p[j] = v[j];
    }
}

template <bool PAIR, bool REC>
__global__ __launch_bounds__(256) void cldice_index_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ skel_x,
                                                           float* __restrict__ skel_y, float* __restrict__ rec_x, unsigned char* __restrict__ sel_x,
                                                           float* __restrict__ rec_y, unsigned char* __restrict__ sel_y, float* __restrict__ part,
                                                           long blocks, long total, int H, int W, int tiles_h, int tiles_w, const CdArgs A) {
    static_assert((CF_TX / 4) * CF_TY == 256, "a strip of four tile positions per thread");
    static_assert(CF_SS % 4 == 0 && CF_SS >= 7 + CF_TX + 2 * CD_MAX_HALO + 1, "the guard columns stay inside a row");
    __shared__ __attribute__((aligned(16))) float pl[2][CF_SR * CF_SS];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<CF_TY, CF_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * H * W;
    const int K = A.K, h = K + 2;
    const int nr = CF_TY + 2 * h, nc = CF_TX + 2 * h;
    const int ox = 4 + ((4 - (h & 3)) & 3);          // cell (r, c) = position (y0 - h + r, x0 - h + c) sits at pl[(r + 1) * CF_SS + c + ox]: the tile at a multiple of four
    const float nan = __builtin_nanf("");
    const int orow = threadIdx.x >> 4, oq = threadIdx.x & 15;           // this thread's strip: row orow of the tile, columns 4 oq .. 4 oq + 3
    const int gy = t.y0 + orow, gx = t.x0 + 4 * oq;
    const int oat = (h + orow + 1) * CF_SS + ox + h + 4 * oq;           // its first cell: a multiple of four
    const int nv = gy < H ? min(4, W - gx) : 0;                           // how many of the strip lie in the image (<= 0: none)
    const bool vec = (W & 3) == 0;
    float sfirst[4] = {0.f, 0.f, 0.f, 0.f}, ufirst[4] = {0.f, 0.f, 0.f, 0.f}, s[4], u0[4];
#pragma unroll 1
    for (int side = 0; side < (PAIR ? 2 : 1); ++side) {
        const float* __restrict__ src = (side ? y : x) + off;
        float* __restrict__ rec = side ? rec_y : rec_x;
        unsigned char* __restrict__ sel = side ? sel_y : sel_x;
        for (int i = threadIdx.x; i < CF_SR * CF_SS; i += 256) {
            const int R = i / CF_SS, r = R - 1, c = i - R * CF_SS - ox;
            const int py = t.y0 - h + r, px = t.x0 - h + c;
            const bool in = (unsigned)r < (unsigned)nr && (unsigned)c < (unsigned)nc && (unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W;
            pl[0][i] = in ? cd_map(src[(long)py * W + px], A) : nan;
        }
        __syncthreads();
        float c[REC ? CD_MAX_ITERS + 1 : 1][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = u0[j] = 0.f;
#pragma unroll
        for (int k = 0; k <= CD_MAX_ITERS; ++k) {
            if (k > K) continue;                      // a fixed trip count, so that the levels unroll and c stays in registers
            const float* __restrict__ cur = pl[k & 1];
            float* __restrict__ nxt = pl[(k & 1) ^ 1];
            // I_{k+1} = E(I_k) on the rows of the tile plus K + 1 - k, the columns of the same widened to whole strips
            const int r0 = k + 1, rows = nr - 2 * (k + 1);
            const int cs = (ox + k + 1) & ~3, strips = ((ox + nc - k - 1 + 3) >> 2) - (cs >> 2);
            for (int it = threadIdx.x; it < rows * strips; it += 256) {
                const int rr = it / strips, q = it - rr * strips;
                const int r = r0 + rr, C = cs + 4 * q;
                const float* __restrict__ p = cur + (r + 1) * CF_SS + C;
                const float4 up = *reinterpret_cast<const float4*>(p - CF_SS), ce = *reinterpret_cast<const float4*>(p),
                             dn = *reinterpret_cast<const float4*>(p + CF_SS);
                const float lf = p[-1], rt = p[4];
                const int py = t.y0 - h + r, px = t.x0 - h + C - ox;
                const bool rin = (unsigned)py < (unsigned)H;
                float4 o;
                o.x = rin && (unsigned)px < (unsigned)W ? cd_min5(up.x, lf, ce.x, ce.y, dn.x) : nan;
                o.y = rin && (unsigned)(px + 1) < (unsigned)W ? cd_min5(up.y, ce.x, ce.y, ce.z, dn.y) : nan;
                o.z = rin && (unsigned)(px + 2) < (unsigned)W ? cd_min5(up.z, ce.y, ce.z, ce.w, dn.z) : nan;
                o.w = rin && (unsigned)(px + 3) < (unsigned)W ? cd_min5(up.w, ce.z, ce.w, rt, dn.w) : nan;
                *reinterpret_cast<float4*>(nxt + (r + 1) * CF_SS + C) = o;
            }
            __syncthreads();
            // this thread's strip: O_k = D(I_{k+1}) from three rows of six values, delta_k, s_k
            float e[3][6];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float* __restrict__ p = nxt + oat + (d - 1) * CF_SS;
                const float4 v = *reinterpret_cast<const float4*>(p);
                e[d][0] = p[-1]; e[d][1] = v.x; e[d][2] = v.y; e[d][3] = v.z; e[d][4] = v.w; e[d][5] = p[4];
            }
            const float4 iv = *reinterpret_cast<const float4*>(cur + oat);
            const float ik[4] = {iv.x, iv.y, iv.z, iv.w};
            float cm[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) cm[i] = cd_max3(e[0][i], e[1][i], e[2][i]);
            float dl[4], tt[4], sp[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float O = cd_max3(cm[j], cm[j + 1], cm[j + 2]);
                const float d = ik[j] - O;
                dl[j] = d > 0.f ? d : 0.f;
                sp[j] = s[j];
                if (k == 0) {
                    u0[j] = ik[j];
                    tt[j] = dl[j];
                    s[j] = dl[j];
                } else {
                    tt[j] = fmaf(-s[j], dl[j], dl[j]);                            // delta_k (1 - s_{k-1}), rounded once
                    s[j] += tt[j] > 0.f ? tt[j] : 0.f;
                }
            }
            if (REC) {
                if (rec != nullptr) {
                    // the arg-min of the cross in I_k and the arg-max of the square in I_{k+1}: the first in row-major order that equals the result
                    const float4 uv = *reinterpret_cast<const float4*>(cur + oat - CF_SS), dv = *reinterpret_cast<const float4*>(cur + oat + CF_SS);
                    const float upv[4] = {uv.x, uv.y, uv.z, uv.w}, dnv[4] = {dv.x, dv.y, dv.z, dv.w};
                    const float row[6] = {cur[oat - 1], ik[0], ik[1], ik[2], ik[3], cur[oat + 4]};
                    unsigned packed = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float m = e[1][j + 1];                                // I_{k+1}[q]
                        const unsigned amin = upv[j] == m ? 0u : row[j] == m ? 1u : row[j + 1] == m ? 2u : row[j + 2] == m ? 3u : 4u;
                        const float O = cd_max3(cm[j], cm[j + 1], cm[j + 2]);
                        unsigned amax = 8u;
#pragma unroll
                        for (int i = 8; i >= 0; --i)
                            if (e[i / 3][j + i % 3] == O) amax = (unsigned)i;
                        packed |= (amin | (amax << 3)) << (8 * j);
                        if (k == 0) {
                            c[0][j] = dl[j] > 0.f ? 1.f : 0.f;
                        } else {
                            const bool mk = tt[j] > 0.f;
                            const float b = mk ? 1.f - dl[j] : 1.f;
#pragma unroll
                            for (int i = 0; i < k; ++i) c[REC ? i : 0][j] *= b;
                            c[REC ? k : 0][j] = (mk && dl[j] > 0.f) ? 1.f - sp[j] : 0.f;
                        }
                    }
                    if (nv > 0) {
                        unsigned char* __restrict__ sp8 = sel + (long)k * total + off + (long)gy * W + gx;
                        if (vec && nv == 4 && (reinterpret_cast<uintptr_t>(sp8) & 3) == 0) {
                            *reinterpret_cast<unsigned*>(sp8) = packed;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (j < nv) sp8[j] = (unsigned char)(packed >> (8 * j));
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (REC && rec != nullptr && nv > 0) {
            float* __restrict__ rp = rec + off + (long)gy * W + gx;
            const bool rvec = vec && (reinterpret_cast<uintptr_t>(rp) & 15) == 0;
#pragma unroll
            for (int k = 0; k <= CD_MAX_ITERS; ++k) {
                if (k > K) continue;
                cd_store4(rp + (long)k * total, c[REC ? k : 0], nv, rvec);
            }
        }
        float* __restrict__ map = side ? skel_y : skel_x;
        if (map != nullptr && nv > 0) {
            float* __restrict__ mp = map + off + (long)gy * W + gx;
            cd_store4(mp, s, nv, vec && (reinterpret_cast<uintptr_t>(mp) & 15) == 0);
        }
        if (PAIR && side == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { sfirst[j] = s[j]; ufirst[j] = u0[j]; }
        }
    }
    if (PAIR) {
        float pxy = 0.f, px = 0.f, pyx = 0.f, py = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nv) {
                pxy = fmaf(sfirst[j], u0[j], pxy);
                px += sfirst[j];
                pyx = fmaf(s[j], ufirst[j], pyx);
                py += s[j];
            }
        }
        block_partial_store_256(pxy, red, part);
        block_partial_store_256(px, red, part + blocks);
        block_partial_store_256(pyx, red, part + 2 * blocks);
        block_partial_store_256(py, red, part + 3 * blocks);
    }
}

// a wave per image; the double scores go behind the partials for cldice_mean
__global__ __launch_bounds__(256) void cldice_final_kernel(const float* __restrict__ part, long blocks, double* __restrict__ dscore, int N, double smooth,
                                                           int average, float* __restrict__ out_image, float* __restrict__ table) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const long per_image = blocks / N;
    const float* __restrict__ p = part + (long)n * per_image;
    double sxy = 0.0, sx = 0.0, syx = 0.0, sy = 0.0;
    for (long i = lane; i < per_image; i += 64) {
        sxy += (double)p[i];
        sx += (double)p[blocks + i];
        syx += (double)p[2 * blocks + i];
        sy += (double)p[3 * blocks + i];
    }
    sxy = wave_sum(sxy);
    sx = wave_sum(sx);
    syx = wave_sum(syx);
    sy = wave_sum(sy);
    const double dp = sx + smooth, dq = sy + smooth;
    const double P = dp > 0.0 ? (sxy + smooth) / dp : 0.0, Q = dq > 0.0 ? (syx + smooth) / dq : 0.0;
    const double PQ = P + Q;
    const double S = PQ != 0.0 ? 2.0 * P * Q / PQ : 0.0;
    if (lane == 0) {
        dscore[n] = S;
        out_image[n] = (float)S;
        if (table != nullptr) {
            const double w = average ? 1.0 / (double)N : 1.0;
            const double SP = PQ != 0.0 ? 2.0 * Q * Q / (PQ * PQ) * w : 0.0, SQ = PQ != 0.0 ? 2.0 * P * P / (PQ * PQ) * w : 0.0;
            table[n] = dp > 0.0 ? (float)(SP / dp) : 0.f;                         // dS / d sum skel(x) u_y
            table[N + n] = dp > 0.0 ? (float)(-SP * P / dp) : 0.f;                // dS / d sum skel(x)
            table[2 * (long)N + n] = dq > 0.0 ? (float)(SQ / dq) : 0.f;           // dS / d sum skel(y) u_x
            table[3 * (long)N + n] = dq > 0.0 ? (float)(-SQ * Q / dq) : 0.f;      // dS / d sum skel(y)
        }
    }
}

__global__ __launch_bounds__(256) void cldice_mean_kernel(const double* __restrict__ dscore, int N, float* __restrict__ out_mean) {
    __shared__ double red[256];
    const double s = block_tree_256(strided_sum_256(dscore, N), red);
    if (threadIdx.x == 0) out_mean[0] = (float)(s / (double)N);
}

// the cells (r, c) of a rows x cols region in flat order, 256 at a time: one division per thread and pass, then steps (64 <= cols)
template <class F>
__device__ __forceinline__ void cd_cells(int rows, int cols, F f) {
    const int sr = 256 / cols, sc = 256 - sr * cols;
    int r = (int)threadIdx.x / cols, c = (int)threadIdx.x - r * cols;
    while (r < rows) {
        f(r, c);
        r += sr;
        c += sc;
        if (c >= cols) { c -= cols; ++r; }
    }
}

// the planes of cldice_grad for a halo of h: (CB_TY + 2 h) x (CB_TX + 2 h) cells, a plane rounded up to whole float4s
static __host__ __device__ __forceinline__ int cd_grad_plane(int h) { return ((CB_TY + 2 * h) * (CB_TX + 2 * h) + 3) & ~3; }

template <bool DICE>
__global__ __launch_bounds__(256) void cldice_grad_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ rec_x,
                                                          const unsigned char* __restrict__ sel_x, const float* __restrict__ rec_y,
                                                          const unsigned char* __restrict__ sel_y, const float* __restrict__ skel_x,
                                                          const float* __restrict__ skel_y, const float* __restrict__ table,
                                                          const float* __restrict__ g, int gN, float* __restrict__ dx, float* __restrict__ dy,
                                                          int N, int C, long total, int H, int W, int tiles_h, int tiles_w, const CdArgs A) {
    static_assert(CB_TX * (CB_TY / 4) == 256, "four rows of a column per thread in the epilogue");
    extern __shared__ __attribute__((aligned(16))) float cd_lds[];
    const PlaneTile t = plane_tile<CB_TY, CB_TX>(tiles_h, tiles_w);
    const long off = (long)t.plane * H * W;
    const int n = t.plane / C;
    const int K = A.K, h = K + 2;
    const int nr = CB_TY + 2 * h, nc = CB_TX + 2 * h;   // cell (r, c) = position (y0 - h + r, x0 - h + c) sits at r * nc + c
    const int PL = cd_grad_plane(h);
    float* __restrict__ G = cd_lds;
    float* __restrict__ D = G + PL;
    float* __restrict__ P0 = D + PL;
    float* __restrict__ P1 = P0 + PL;
    unsigned char* __restrict__ SEL = reinterpret_cast<unsigned char*>(P1 + PL);
    const float up = DICE ? g[gN > 1 ? n : 0] : 0.f;
#pragma unroll 1
    for (int side = 0; side < (DICE ? 2 : 1); ++side) {
        float* __restrict__ out = side ? dy : dx;
        if (out == nullptr) continue;
        const float* __restrict__ other = (side ? x : y);
        const float* __restrict__ rec = side ? rec_y : rec_x;
        const unsigned char* __restrict__ sel = side ? sel_y : sel_x;
        float alpha = 0.f, beta = 0.f, gamma = 0.f;
        if (DICE) {
            alpha = table[(side ? 2L : 0L) * N + n] * up;
            beta = table[(side ? 3L : 1L) * N + n] * up;
            gamma = table[(side ? 0L : 2L) * N + n] * up;
        }
        // the cotangent of this side's skeleton on the tile plus K + 2, 0 beyond the image; nothing stands in the two carried planes yet
        cd_cells(nr, nc, [&](int r, int c) {
            const int py = t.y0 - h + r, px = t.x0 - h + c;
            float v = 0.f;
            if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) {
                const long at = off + (long)py * W + px;
                v = DICE ? fmaf(alpha, cd_map(other[at], A), beta) : g[at];
            }
            G[r * nc + c] = v;
            P0[r * nc + c] = 0.f;
            P1[r * nc + c] = 0.f;
        });
        __syncthreads();
        float* __restrict__ X = P0;                   // what the level above left; becomes Ibar_{k+1} in place
        float* __restrict__ Y = P1;
#pragma unroll 1
        for (int k = K; k >= 0; --k) {
            // dbar_k = G c_k and the selection bytes on the tile plus k + 2
            {
                const int m = k + 2, r0 = h - m, rows = CB_TY + 2 * m, cols = CB_TX + 2 * m;
                const float* __restrict__ rk = rec + (long)k * total + off;
                const unsigned char* __restrict__ sk = sel + (long)k * total + off;
                cd_cells(rows, cols, [&](int rr, int cc) {
                    const int r = r0 + rr, c = r0 + cc;
                    const int py = t.y0 - h + r, px = t.x0 - h + c;
                    float v = 0.f;
                    unsigned char b = CD_NONE;
                    if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) {
                        const long at = (long)py * W + px;
                        v = G[r * nc + c] * rk[at];
                        b = sk[at];
                    }
                    D[r * nc + c] = v;
                    SEL[r * nc + c] = b;
                });
            }
            __syncthreads();
            // Ibar_{k+1}[p] on the tile plus k + 1: minus dbar_k of the q of p's square whose maximum was taken at p
            {
                const int m = k + 1, r0 = h - m, rows = CB_TY + 2 * m, cols = CB_TX + 2 * m;
                cd_cells(rows, cols, [&](int rr, int cc) {
                    const int at = (r0 + rr) * nc + r0 + cc;
                    float acc = X[at];
#pragma unroll
                    for (int d = 0; d < 9; ++d) {                                 // a fixed order, and no branch: what is not routed here subtracts 0
                        const int q = at + (d / 3 - 1) * nc + (d % 3 - 1);
                        acc -= (SEL[q] >> 3) == 8 - d ? D[q] : 0.f;
                    }
                    X[at] = acc;
                });
            }
            __syncthreads();
            // what level k leaves at p on the tile plus k: dbar_k[p] plus Ibar_{k+1} of the r of p's cross whose minimum was taken at p
            {
                const int r0 = h - k, rows = CB_TY + 2 * k, cols = CB_TX + 2 * k;
                cd_cells(rows, cols, [&](int rr, int cc) {
                    const int at = (r0 + rr) * nc + r0 + cc;
                    float acc = D[at];
                    const int nb[5] = {at - nc, at - 1, at, at + 1, at + nc};
#pragma unroll
                    for (int d = 0; d < 5; ++d) acc += (SEL[nb[d]] & 7) == 4 - d ? X[nb[d]] : 0.f;
                    Y[at] = acc;
                });
            }
            __syncthreads();
            float* __restrict__ sw = X; X = Y; Y = sw;
        }
        // X holds the gradient by u on the tile
        const int col = threadIdx.x & 63, r4 = 4 * (threadIdx.x >> 6);
        const int gx = t.x0 + col;
        const float* __restrict__ sko = side ? skel_x : skel_y;
        if (gx < W) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gy = t.y0 + r4 + j;
                if (gy < H) {
                    const long at = off + (long)gy * W + gx;
                    float v = X[(h + r4 + j) * nc + h + col];
                    if (DICE) v = fmaf(gamma, sko[at], v);
                    out[at] = (A.sgn * v) / A.range;
                }
            }
        }
        __syncthreads();
    }
}

static int cd_shape(const char* what, long N, long C, int H, int W) {
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL || N * C > 0x7fffffffL || H < 1 || W < 1)
        return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld images of %ld channels of %d x %d)", what, N, C, H, W);
    if ((long)H * W > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: a plane of %d x %d exceeds 2^31 - 1 samples", what, H, W);
    return FAOCTASR_OK;
}

static int cd_tiles(const char* what, long planes, int H, int W, int TY, int TX, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, H, W, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

static int cd_args(const char* what, int iters, float lo, float hi, int bright, CdArgs* A) {
    if (iters < 1 || iters > CD_MAX_ITERS) return fail(FAOCTASR_EINVAL, "%s: iters %d (1..%d)", what, iters, CD_MAX_ITERS);
    if (!(hi > lo) || !(hi - lo < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: value_range (%g, %g) must be finite with hi > lo", what, (double)lo, (double)hi);
    A->K = iters;
    A->lo = bright ? lo : hi;
    A->range = hi - lo;
    A->sgn = bright ? 1.f : -1.f;
    return FAOCTASR_OK;
}

static long cd_even(long v) { return (v + 1) & ~1L; }

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_cldice_workspace_floats(long N, long C, int H, int W) {
    int th, tw;
    long blocks;
    if (cd_shape("cldice_workspace_floats", N, C, H, W) || cd_tiles("cldice_workspace_floats", N * C, H, W, CF_TY, CF_TX, &th, &tw, &blocks)) return -1;
    return cd_even(4 * blocks) + 2 * N;
}

extern "C" int faoctasr_cldice_index(const float* x, const float* y, float* skel_x, float* skel_y, float* rec_x, unsigned char* sel_x, float* rec_y,
                                     unsigned char* sel_y, float* workspace, long N, long C, int H, int W, int iters, float lo, float hi,
                                     int bright, faoctasr_stream_t stream) {
    if (!x) return fail(FAOCTASR_EINVAL, "cldice_index: null pointer");
    if ((rec_x == nullptr) != (sel_x == nullptr) || (rec_y == nullptr) != (sel_y == nullptr))
        return fail(FAOCTASR_EINVAL, "cldice_index: a side's records come as a pair (the floats and the selection bytes) or not at all");
    if (y ? !workspace : (!skel_x || skel_y || rec_y || workspace))
        return fail(FAOCTASR_EINVAL, "cldice_index: a pair takes a workspace; one image takes its skeleton map, its records or none, and nothing else");
    int rc, th, tw;
    long blocks;
    CdArgs A;
    if ((rc = cd_shape("cldice_index", N, C, H, W))) return rc;
    if ((rc = cd_args("cldice_index", iters, lo, hi, bright, &A))) return rc;
    if ((rc = cd_tiles("cldice_index", N * C, H, W, CF_TY, CF_TX, &th, &tw, &blocks))) return rc;
    const long total = N * C * (long)H * W;
    const bool recs = rec_x || rec_y;
#define CD_LAUNCH(PAIR, REC)                                                                                                                      \
    hipLaunchKernelGGL((cldice_index_kernel<PAIR, REC>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, skel_x, skel_y, rec_x, sel_x, \
                       rec_y, sel_y, workspace, blocks, total, H, W, th, tw, A)
    if (y) {
        if (recs) CD_LAUNCH(true, true); else CD_LAUNCH(true, false);
    } else {
        if (recs) CD_LAUNCH(false, true); else CD_LAUNCH(false, false);
    }
#undef CD_LAUNCH
    return check_launch("cldice_index");
}

extern "C" int faoctasr_cldice_final(float* workspace, long N, long C, int H, int W, double smooth, int average, float* out_image, float* out_mean,
                                     float* table, faoctasr_stream_t stream) {
    if (!workspace || !out_image) return fail(FAOCTASR_EINVAL, "cldice_final: null pointer");
    if (!(smooth >= 0.0) || !(smooth < (double)INFINITY)) return fail(FAOCTASR_EINVAL, "cldice_final: smooth %g must be finite and >= 0", smooth);
    int rc, th, tw;
    long blocks;
    if ((rc = cd_shape("cldice_final", N, C, H, W))) return rc;
    if ((rc = cd_tiles("cldice_final", N * C, H, W, CF_TY, CF_TX, &th, &tw, &blocks))) return rc;
    double* dscore = reinterpret_cast<double*>(workspace + cd_even(4 * blocks));
    if ((reinterpret_cast<uintptr_t>(dscore) & 7) != 0) return fail(FAOCTASR_EINVAL, "cldice_final: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(cldice_final_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, workspace, blocks, dscore, (int)N, smooth,
                       average, out_image, table);
    if ((rc = check_launch("cldice_final"))) return rc;
    if (out_mean) {
        hipLaunchKernelGGL(cldice_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dscore, (int)N, out_mean);
        rc = check_launch("cldice_final");
    }
    return rc;
}

extern "C" int faoctasr_cldice_grad(const float* x, const float* y, const float* rec_x, const unsigned char* sel_x, const float* rec_y,
                                    const unsigned char* sel_y, const float* skel_x, const float* skel_y, const float* table, const float* g, int gN,
                                    float* dx, float* dy, long N, long C, int H, int W, int iters, float lo, float hi, int bright,
                                    faoctasr_stream_t stream) {
    if (!g) return fail(FAOCTASR_EINVAL, "cldice_grad: null pointer");
    const bool dice = table != nullptr;
    if (dice ? (!x || !y || (!dx && !dy) || (dx && (!rec_x || !sel_x || !skel_y)) || (dy && (!rec_y || !sel_y || !skel_x)))
             : (!dx || !rec_x || !sel_x || dy || rec_y || sel_y))
        return fail(FAOCTASR_EINVAL, "cldice_grad: the index form takes both images, the table and per wanted side its records and the other side's "
                                     "skeleton map; the map form the records of x, g and dx");
    if (dice && gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "cldice_grad: gN must be 1 or N");
    int rc, th, tw;
    long blocks;
    CdArgs A;
    if ((rc = cd_shape("cldice_grad", N, C, H, W))) return rc;
    if ((rc = cd_args("cldice_grad", iters, lo, hi, bright, &A))) return rc;
    if ((rc = cd_tiles("cldice_grad", N * C, H, W, CB_TY, CB_TX, &th, &tw, &blocks))) return rc;
    const long total = N * C * (long)H * W;
    const size_t lds = (size_t)CB_CELL_BYTES * cd_grad_plane(iters + 2);          // 59,840 bytes at iters = 10: below the 64 KiB that need no opt-in
    static_assert((size_t)CB_CELL_BYTES * (((CB_TY + 2 * CD_MAX_HALO) * (CB_TX + 2 * CD_MAX_HALO) + 3) & ~3) <= 65536, "cldice_grad's planes fit 64 KiB");
    if (dice)
        hipLaunchKernelGGL(cldice_grad_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, y, rec_x, sel_x, rec_y, sel_y, skel_x,
                           skel_y, table, g, gN, dx, dy, (int)N, (int)C, total, H, W, th, tw, A);
    else
        hipLaunchKernelGGL(cldice_grad_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x, y, rec_x, sel_x, rec_y, sel_y, skel_x,
                           skel_y, table, g, gN, dx, dy, (int)N, (int)C, total, H, W, th, tw, A);
    return check_launch("cldice_grad");
}
