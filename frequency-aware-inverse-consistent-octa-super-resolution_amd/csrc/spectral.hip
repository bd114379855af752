// Spectral phase-consistency loss (model.py:36-58 of the reference) on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
//
//   m[u,v] = 1 - exp(-0.5 (u_c^2 + v_c^2) / radius^2)           u_c, v_c: centred frequency of the UNSHIFTED bin,
//   a_x    = m * log|fft2(x)|  over (C,H,W)                      u_c = ((u + H/2) mod H) - H/2 (the reference's fftshift is the
//   loss   = -<a_x, a_y> / (|a_x| |a_y|)                         same permutation on both operands of a dot product: dropped)
//
// The DFT of a real image is four real GEMMs with the symmetric tables C_n[k,l] = cos(2 pi kl/n), S_n = sin(2 pi kl/n):
//   [P | Q] = X [C_W | S_W]                  row pass    (faoctasr_sgemm_batched, x and y in one launch)
//   Re = C_H P - S_H Q,  J = S_H P + C_H Q   column pass (J = -Im; only Re^2 + J^2 and the pair's gradient are ever used)
// The column pass accumulates Re and J of the x image and the y image of one (sample, channel) in the same block, forms
// a = m * 0.5 * log(Re^2 + J^2) in the accumulator registers and reduces <a_x,a_y>, |a_x|^2, |a_y|^2 over its tile: the spectrum
// makes no separate trip through memory for abs / log / mul / flatten.  One partial triple per block goes to the workspace with
// plain stores; a finishing kernel adds them in a fixed order in double (no float atomics: the loss is bit-reproducible).
//
// Saved for the backward: Re and J, 8 bytes per pixel and image (512 KiB per 256x256 image); the backward recomputes m and a.
//   dRe = g * dloss/da * m * Re / |F|^2,  dJ likewise,  dloss/da_x = -(a_y / (|a_x||a_y|) - <a_x,a_y> a_x / (|a_x|^3 |a_y|))
//   [T1 | T2] = [C_H dRe + S_H dJ | C_H dJ - S_H dRe]            fused with the formation of dRe, dJ (one kernel)
//   dX = [T1 | T2] [C_W ; S_W]                                   one more faoctasr_sgemm_batched, K = 2W
//
// A bin whose amplitude is exactly zero gives log 0 = -inf and a NaN loss, as in the reference: no clamp, no epsilon (either
// would change the value everywhere).
//
// Block 256 threads, output tile 64x64, K chunk 16; waves 2x2, four 32x32 accumulators each (Re_x, J_x, Re_y, J_y).
//
// The focal frequency loss (second half of this file) runs on the same tables, row pass and tile, with two accumulators.
// The spectral-profile loss (third section) runs them on the half spectrum: columns 0..W/2 only, both GEMM passes half as wide.
// The Fourier ring correlation (fourth section) is that path with both transforms kept complex and three ring sums in place of one.
// Phase correlation and the Fourier shift (fifth section) add the way back: the half-spectrum inverse as a forward pass.
#include <cstdint>
#include "common.h"

namespace faoctasr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PH_KC = 16, PH_T = 64;

__device__ __forceinline__ int centred(int u, int n) { return (u + n / 2) % n - n / 2; }

// the reference builds its mask in double and rounds it to float once
__device__ __forceinline__ float phase_mask(int uc, int vc, double inv2r2) {
    return (float)(1.0 - exp(-(double)(uc * uc + vc * vc) * inv2r2));
}

// out[0, 2n^2): [C_n | S_n], n rows of 2n;  out[2n^2, 4n^2): [C_n ; S_n], 2n rows of n.  Phase reduced mod n in integers.
__global__ __launch_bounds__(256) void dft_tables_kernel(float* __restrict__ out, int n) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * n) return;
    const int k = (int)(e / n), l = (int)(e % n);
    const long ph = ((long)k * l) % n;
    const double t = 2.0 * (double)ph / (double)n;
    const float c = (float)cospi(t), s = (float)sinpi(t);
    out[(long)k * 2 * n + l] = c;
    out[(long)k * 2 * n + n + l] = s;
    float* st = out + 2L * n * n;
    st[e] = c;
    st[(long)n * n + e] = s;
}

struct PhaseWs {
    double* stats;      // [N][4]: <a_x,a_y>, |a_x|^2, |a_y|^2, unused
    float* part;        // [N*C][tiles][3]
    float* planes;      // [2 (x,y)][N*C][2 (Re,J)][H][W]
    float* pq;          // [2 (x,y)][N*C][H][2W]: [P | Q] in the forward, [T1 | T2] in the backward
    long total;
};

static PhaseWs phase_ws(float* ws, long N, long C, long H, long W) {
    PhaseWs p;
    const long tiles = ((H + PH_T - 1) / PH_T) * ((W + PH_T - 1) / PH_T);
    long off = 0;
    p.stats = (double*)ws;
    off += 8 * N;
    p.part = ws + off;
    off += 3 * N * C * tiles;
    off = (off + 3) & ~3L;
    p.planes = ws + off;
    off += 4 * N * C * H * W;
    p.pq = ws + off;
    off += 4 * N * C * H * W;
    p.total = off;
    return p;
}

// stage one 16 x 64 chunk of the symmetric tables: rows k0.. of [C_H | S_H], columns r0.. (C_H[r][k] = C_H[k][r])
__device__ __forceinline__ void stage_tables(float* Cs, float* Ss, const float* __restrict__ tabH, int H, int k0, int r0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int k = k0 + (e >> 6), r = r0 + (e & 63);
        const bool ok = k < H && r < H;
        Cs[e] = ok ? tabH[(long)k * 2 * H + r] : 0.f;
        Ss[e] = ok ? tabH[(long)k * 2 * H + H + r] : 0.f;
    }
}

__global__ __launch_bounds__(256) void phase_col_fwd_kernel(const float* __restrict__ pq, const float* __restrict__ tabH,
                                                            float* __restrict__ planes, float* __restrict__ part, int H, int W,
                                                            long imgs, double inv2r2) {
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    __shared__ float red[12];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int u0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const float* pqx = pq + img * H * 2 * W;
    const float* pqy = pq + (imgs + img) * H * 2 * W;
    f32x16 rx, jx, ry, jy;
#pragma unroll
    for (int r = 0; r < 16; ++r) rx[r] = jx[r] = ry[r] = jy[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, u0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int k = k0 + (e >> 6), v = v0 + (e & 63);
            const bool ok = k < H && v < W;
            const long o = (long)k * 2 * W + v;
            Bs[0][e] = ok ? pqx[o] : 0.f;
            Bs[1][e] = ok ? pqx[o + W] : 0.f;
            Bs[2][e] = ok ? pqy[o] : 0.f;
            Bs[3][e] = ok ? pqy[o + W] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float px = Bs[0][bo], qx = Bs[1][bo], py = Bs[2][bo], qy = Bs[3][bo];
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, px, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(as, px, jx, 0, 0, 0);
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, py, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(as, py, jy, 0, 0, 0);
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qx, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qx, jx, 0, 0, 0);
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qy, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qy, jy, 0, 0, 0);
        }
    }
    // epilogue: a = m * 0.5 * log(Re^2 + J^2) for both images, the three sums, Re and J for the backward
    const int v = v0 + wn * 32 + l31;
    float dot = 0.f, nx = 0.f, ny = 0.f;
    if (v < W) {
        const int vc = centred(v, W);
        const long hw = (long)H * W;
        float* plx = planes + img * 2 * hw;
        float* ply = planes + (imgs + img) * 2 * hw;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int u = u0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (u < H) {
                const float m = phase_mask(centred(u, H), vc, inv2r2);
                const float ax = m * 0.5f * logf(rx[rr] * rx[rr] + jx[rr] * jx[rr]);
                const float ay = m * 0.5f * logf(ry[rr] * ry[rr] + jy[rr] * jy[rr]);
                dot += ax * ay;
                nx += ax * ax;
                ny += ay * ay;
                const long o = (long)u * W + v;
                plx[o] = rx[rr];
                plx[hw + o] = jx[rr];
                ply[o] = ry[rr];
                ply[hw + o] = jy[rr];
            }
        }
    }
    dot = wave_sum(dot);
    nx = wave_sum(nx);
    ny = wave_sum(ny);
    if (lane == 0) {
        red[wave * 3 + 0] = dot;
        red[wave * 3 + 1] = nx;
        red[wave * 3 + 2] = ny;
    }
    __syncthreads();
    if (tid < 3) {
        const long tile = (long)blockIdx.y * gridDim.x + blockIdx.x, tiles = (long)gridDim.x * gridDim.y;
        part[(img * tiles + tile) * 3 + tid] = (red[tid] + red[3 + tid]) + (red[6 + tid] + red[9 + tid]);
    }
}

// one thread per sample adds that sample's partial triples in a fixed order (double), keeps the sums for the backward and writes
// the loss; thread 0 then averages the per-sample losses in index order
__global__ __launch_bounds__(64) void phase_finish_kernel(const float* __restrict__ part, double* __restrict__ stats,
                                                          float* __restrict__ loss_per_sample, float* __restrict__ loss_mean, int N,
                                                          long per_sample) {
    for (int b = threadIdx.x; b < N; b += 64) {
        const float* p = part + (long)b * per_sample * 3;
        double d = 0.0, sx = 0.0, sy = 0.0;
        for (long i = 0; i < per_sample; ++i) {
            d += (double)p[3 * i];
            sx += (double)p[3 * i + 1];
            sy += (double)p[3 * i + 2];
        }
        stats[4 * b] = d;
        stats[4 * b + 1] = sx;
        stats[4 * b + 2] = sy;
        stats[4 * b + 3] = 0.0;
        const double eps = 1e-8;                             // torch.cosine_similarity's default
        loss_per_sample[b] = (float)(-d / (fmax(sqrt(sx), eps) * fmax(sqrt(sy), eps)));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < N; ++b) s += (double)loss_per_sample[b];
        *loss_mean = (float)(s / (double)N);
    }
}

// [T1 | T2] = [C_H dRe + S_H dJ | C_H dJ - S_H dRe] for the x image (want_x) and / or the y image (want_y) of one
// (sample, channel); dRe, dJ are formed from the saved planes while they are staged into LDS
__global__ __launch_bounds__(256) void phase_col_bwd_kernel(const float* __restrict__ planes, const float* __restrict__ tabH,
                                                            const double* __restrict__ stats, const float* __restrict__ g,
                                                            float* __restrict__ T, int H, int W, int C, int N, long imgs, double inv2r2,
                                                            int want_x, int want_y) {
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int h0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const long hw = (long)H * W;
    const float* plx = planes + img * 2 * hw;
    const float* ply = planes + (imgs + img) * 2 * hw;
    // dloss/da_x = -(k1 a_y - k2x a_x), dloss/da_y = -(k1 a_x - k2y a_y), times the incoming gradient of the batch mean
    const double* st = stats + 4 * (img / C);
    const double eps = 1e-8;
    const double d = st[0], sx = fmax(sqrt(st[1]), eps), sy = fmax(sqrt(st[2]), eps);
    const double k1d = 1.0 / (sx * sy);
    const float gs = g[0] / (float)N;
    const float k1 = (float)k1d, k2x = (float)(d / (sx * sx) * k1d), k2y = (float)(d / (sy * sy) * k1d);
    const int sv = v0 + (tid & 63);
    const int svc = centred(sv < W ? sv : 0, W);
    f32x16 t1x, t2x, t1y, t2y;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1x[r] = t2x[r] = t1y[r] = t2y[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, h0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int u = k0 + (e >> 6);
            float drx = 0.f, djx = 0.f, dry = 0.f, djy = 0.f;
            if (u < H && sv < W) {
                const long o = (long)u * W + sv;
                const float Rx = plx[o], Jx = plx[hw + o], Ry = ply[o], Jy = ply[hw + o];
                const float fx = Rx * Rx + Jx * Jx, fy = Ry * Ry + Jy * Jy;
                const float m = phase_mask(centred(u, H), svc, inv2r2);
                const float ax = m * 0.5f * logf(fx), ay = m * 0.5f * logf(fy);
                const float wx = -gs * (k1 * ay - k2x * ax) * m / fx;
                const float wy = -gs * (k1 * ax - k2y * ay) * m / fy;
                drx = wx * Rx;
                djx = wx * Jx;
                dry = wy * Ry;
                djy = wy * Jy;
            }
            Bs[0][e] = drx;
            Bs[1][e] = djx;
            Bs[2][e] = dry;
            Bs[3][e] = djy;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            if (want_x) {
                const float dr = Bs[0][bo], dj = Bs[1][bo];
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2x, 0, 0, 0);
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2x, 0, 0, 0);
            }
            if (want_y) {
                const float dr = Bs[2][bo], dj = Bs[3][bo];
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2y, 0, 0, 0);
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2y, 0, 0, 0);
            }
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < W) {
        float* Tx = T + img * H * 2 * W;
        float* Ty = T + (imgs + img) * H * 2 * W;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = h0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (h < H) {
                const long o = (long)h * 2 * W + v;
                if (want_x) {
                    Tx[o] = t1x[rr];
                    Tx[o + W] = t2x[rr];
                }
                if (want_y) {
                    Ty[o] = t1y[rr];
                    Ty[o + W] = t2y[rr];
                }
            }
        }
    }
}

static int phase_check(const char* what, const void* ws, int N, int C, int H, int W, float radius) {
    if (N < 1 || C < 1 || H < 2 || W < 2) return fail(FAOCTASR_EINVAL, "%s: bad shape N %d C %d H %d W %d (H, W >= 2)", what, N, C, H, W);
    if (H > 8192 || W > 8192) return fail(FAOCTASR_EUNSUPPORTED, "%s: H %d, W %d > 8192", what, H, W);
    if ((long)N * C > 65535) return fail(FAOCTASR_EUNSUPPORTED, "%s: N*C %ld > 65535", what, (long)N * C);
    if ((long)N * C * H > (1L << 21)) return fail(FAOCTASR_EUNSUPPORTED, "%s: N*C*H %ld > 2^21", what, (long)N * C * H);
    if (!(radius > 0.f)) return fail(FAOCTASR_EINVAL, "%s: radius %g must be positive", what, (double)radius);
    if ((uintptr_t)ws & 7) return fail(FAOCTASR_EINVAL, "%s: workspace must be 8-byte aligned", what);
    return FAOCTASR_OK;
}


// ---- focal frequency loss (Jiang, Dai, Wu, Loy, ICCV 2021) -----------------------------------------------------------------
//   D = fft2(x, ortho) - fft2(y, ortho) = fft2(x - y, ortho),  q = |D|^2,  w = phi(q) / phi(M),  L = mean(w q)
//   phi(q) = q^(alpha/2) or log(q^(alpha/2) + 1),  M = max q over the plane (or the batch); w is a constant for the gradient.
// One spectrum per image PAIR: the column pass stages P_x - P_y and Q_x - Q_y, so a wave tile carries two accumulators (Re, J).
// The weight's normaliser factorises out of the sum, sum w q = (sum phi(q) q) / phi(M): one pass, a partial sum and a partial
// maximum per block, and the finishing kernel divides.  dL/dx = (2/count) Re ifft2(w D, ortho) = -dL/dy: one transform per backward.
struct FflWs {
    double* stats;      // [N*C][2]: sum phi(q) q, max q
    float* part;        // [N*C][tiles][2]
    float* pq;          // [2 (x,y)][N*C][H][2W]: [P | Q] in the forward; its first half is [T1 | T2] in the backward
    long total;
};

static FflWs ffl_ws(float* ws, long N, long C, long H, long W) {
    FflWs p;
    const long tiles = ((H + PH_T - 1) / PH_T) * ((W + PH_T - 1) / PH_T);
    long off = 0;
    p.stats = (double*)ws;
    off += 4 * N * C;
    p.part = ws + off;
    off += 2 * N * C * tiles;
    off = (off + 3) & ~3L;
    p.pq = ws + off;
    off += 4 * N * C * H * W;
    p.total = off;
    return p;
}

enum { FFL_ONE = 0, FFL_SQRT = 1, FFL_ID = 2, FFL_POW = 3 };

// phi(q): the exact forms for alpha = 0, 1, 2 (0^0 = 1, as torch.pow), powf otherwise
__device__ __forceinline__ float ffl_phi(float q, int form, float half_alpha, int logm) {
    float w;
    switch (form) {
        case FFL_ONE: w = 1.f; break;
        case FFL_SQRT: w = sqrtf(q); break;
        case FFL_ID: w = q; break;
        default: w = powf(q, half_alpha); break;
    }
    return logm ? log1pf(w) : w;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// column pass of the difference spectrum: Re = s (C_H P - S_H Q), J = s (S_H P + C_H Q) with P = P_x - P_y, Q = Q_x - Q_y formed
// while staging and s = 1/sqrt(HW); q = Re^2 + J^2 in the accumulator registers; one partial (sum phi(q) q, max q) per block.
// planes == nullptr: no gradient is wanted and the spectrum is not stored.
__global__ __launch_bounds__(256) void ffl_col_fwd_kernel(const float* __restrict__ pq, const float* __restrict__ tabH,
                                                          float* __restrict__ planes, float* __restrict__ part, int H, int W, long imgs,
                                                          float scale, int form, float half_alpha, int logm) {
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[2][PH_KC * PH_T];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int u0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const float* pqx = pq + img * H * 2 * W;
    const float* pqy = pq + (imgs + img) * H * 2 * W;
    f32x16 re, jm;
#pragma unroll
    for (int r = 0; r < 16; ++r) re[r] = jm[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, u0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int k = k0 + (e >> 6), v = v0 + (e & 63);
            const bool ok = k < H && v < W;
            const long o = (long)k * 2 * W + v;
            Bs[0][e] = ok ? pqx[o] - pqy[o] : 0.f;
            Bs[1][e] = ok ? pqx[o + W] - pqy[o + W] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float p = Bs[0][bo], q = Bs[1][bo];
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, p, re, 0, 0, 0);
            jm = __builtin_amdgcn_mfma_f32_32x32x2f32(as, p, jm, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, q, re, 0, 0, 0);
            jm = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, q, jm, 0, 0, 0);
        }
    }
    // epilogue: lanes outside the plane (remainder tiles) add 0 to the sum and to the maximum (q >= 0)
    const int v = v0 + wn * 32 + l31;
    float sum = 0.f, mx = 0.f;
    if (v < W) {
        const long hw = (long)H * W;
        float* pl = planes ? planes + img * 2 * hw : nullptr;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int u = u0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (u < H) {
                const float r = re[rr] * scale, j = jm[rr] * scale;
                const float q = r * r + j * j;
                sum += ffl_phi(q, form, half_alpha, logm) * q;
                mx = fmaxf(mx, q);
                if (pl) {
                    const long o = (long)u * W + v;
                    pl[o] = r;
                    pl[hw + o] = j;
                }
            }
        }
    }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if (lane == 0) {
        red[wave] = sum;
        red[4 + wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        const long tile = (long)blockIdx.y * gridDim.x + blockIdx.x, tiles = (long)gridDim.x * gridDim.y;
        float* o = part + (img * tiles + tile) * 2;
        o[0] = (red[0] + red[1]) + (red[2] + red[3]);
        o[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    }
}

__device__ __forceinline__ double ffl_phi_d(double q, int form, double half_alpha, int logm) {
    double w;
    switch (form) {
        case FFL_ONE: w = 1.0; break;
        case FFL_SQRT: w = sqrt(q); break;
        case FFL_ID: w = q; break;
        default: w = pow(q, half_alpha); break;
    }
    return logm ? log1p(w) : w;
}

// single block.  Thread t owns planes t, t + 256, ...: it adds a plane's partial sums in index order in double and takes its
// maximum; the block reduces the maxima over the batch (batch_matrix); every plane's sum is divided by phi(M) (a plane with
// M = 0 adds exactly 0) and the quotients are added per thread in plane order, then over the threads by a fixed tree.
// inv_phi (may be nullptr) keeps 1 / phi(M) per plane (0 where phi(M) = 0) for the backward.
__global__ __launch_bounds__(256) void ffl_finish_kernel(const float* __restrict__ part, double* __restrict__ stats,
                                                         float* __restrict__ inv_phi, float* __restrict__ loss, long imgs, long tiles,
                                                         double count, int form, double half_alpha, int logm, int batch) {
    __shared__ double red[256];
    __shared__ float mxs[256];
    const int tid = threadIdx.x;
    float tmax = 0.f;
    for (long p = tid; p < imgs; p += 256) {
        const float* q = part + p * tiles * 2;
        double s = 0.0;
        float m = 0.f;
        for (long i = 0; i < tiles; ++i) {
            s += (double)q[2 * i];
            m = fmaxf(m, q[2 * i + 1]);
        }
        stats[2 * p] = s;
        stats[2 * p + 1] = (double)m;
        tmax = fmaxf(tmax, m);
    }
    mxs[tid] = tmax;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) mxs[tid] = fmaxf(mxs[tid], mxs[tid + o]);
        __syncthreads();
    }
    const double mall = (double)mxs[0];
    double acc = 0.0;
    for (long p = tid; p < imgs; p += 256) {
        const double ph = ffl_phi_d(batch ? mall : stats[2 * p + 1], form, half_alpha, logm);
        const bool ok = ph > 0.0;
        if (inv_phi) inv_phi[p] = ok ? (float)(1.0 / ph) : 0.f;
        if (ok) acc += stats[2 * p] / ph;
    }
    acc = block_tree_256(acc, red);
    if (tid == 0) *loss = (float)(acc / count);
}

// [T1 | T2] = [C_H dRe + S_H dJ | C_H dJ - S_H dRe] with (dRe, dJ) = g * coef * phi(q) / phi(M) * (Re, J) formed from the saved
// planes while they are staged; coef = +-2 / (count sqrt(HW)) carries the mean, the ortho scale and the side (dx: +, dy: -)
__global__ __launch_bounds__(256) void ffl_col_bwd_kernel(const float* __restrict__ planes, const float* __restrict__ inv_phi,
                                                          const float* __restrict__ tabH, const float* __restrict__ g,
                                                          float* __restrict__ T, int H, int W, float coef, int form, float half_alpha,
                                                          int logm) {
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[2][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int h0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const long hw = (long)H * W;
    const float* pl = planes + img * 2 * hw;
    const float gs = g[0] * coef, ip = inv_phi[img];
    const int sv = v0 + (tid & 63);
    f32x16 t1, t2;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1[r] = t2[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, h0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int u = k0 + (e >> 6);
            float dr = 0.f, dj = 0.f;
            if (u < H && sv < W) {
                const long o = (long)u * W + sv;
                const float R = pl[o], J = pl[hw + o];
                const float w = gs * (ffl_phi(R * R + J * J, form, half_alpha, logm) * ip);
                dr = w * R;
                dj = w * J;
            }
            Bs[0][e] = dr;
            Bs[1][e] = dj;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float dr = Bs[0][bo], dj = Bs[1][bo];
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1, 0, 0, 0);
            t2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1, 0, 0, 0);
            t2 = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2, 0, 0, 0);
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < W) {
        float* To = T + img * H * 2 * W;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = h0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (h < H) {
                const long o = (long)h * 2 * W + v;
                To[o] = t1[rr];
                To[o + W] = t2[rr];
            }
        }
    }
}

// the second gradient of the focal frequency loss: dy = -dx, exactly
__global__ __launch_bounds__(256) void negate_kernel(const float* __restrict__ a, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = -a[i];
}

static int ffl_check(const char* what, const void* ws, int N, int C, int H, int W, float alpha) {
    int rc = phase_check(what, ws, N, C, H, W, 1.f);
    if (rc) return rc;
    if (!(alpha >= 0.f) || alpha > 3.0e38f) return fail(FAOCTASR_EINVAL, "%s: alpha %g must be finite and >= 0", what, (double)alpha);
    return FAOCTASR_OK;
}

static int ffl_form(float alpha) { return alpha == 0.f ? FFL_ONE : alpha == 1.f ? FFL_SQRT : alpha == 2.f ? FFL_ID : FFL_POW; }


// ---- spectral-profile loss (after Durall, Keuper, Keuper, CVPR 2020) --------------------------------------------------------------
//   q = |fft2(x)|^2 / (HW),  A[k] = mean of q over the ring bin(u,v) = floor(M sqrt(u_c^2/H^2 + v_c^2/W^2)) = k,  M = min(H, W),
//   a = log(A + eps);  L = mean_{n,c,k>=k_min} (a_x - a_y)^2, or on the batch means of a (the unpaired, domain form).
// |F|^2 of a real image is point-symmetric and so is bin(u,v): only the columns v < Wh = W/2 + 1 are transformed, a column counting
// m_v = 2 times unless it is its own mirror (v = 0, and v = W/2 for even W).  Both GEMM passes are half as wide as the other two
// losses', forward and backward:
//   [P | Q] = X [C_W[:, :Wh] | S_W[:, :Wh]]        row pass, W x 2Wh half tables (the caller's, cut from faoctasr_dft_tables)
//   Re, J as above on H x Wh;  pw = m_v (Re^2 + J^2) / (HW)   formed in the accumulator registers
//   A[k] = (1 / cnt_k) sum of pw over the bin      a gather along a host-built CSR list (the geometry is fixed): no atomics
//   finish (one block, double, fixed order): logs, batch means, loss, and coef[p][k] = dL/dA[p,k] / cnt_k for the backward
//   (dRe, dJ) = g (2/(HW)) m_v coef[p][bin] (Re, J) formed while staging;  [T1 | T2] as above;  dX = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]
// x and y run one instruction sequence each (L(x,y) == L(y,x) bit for bit); the epilogues are compiled without contraction.
// Wh == W (a measuring switch of tools/sprof_bench.py) runs the same kernels on the full spectrum with every m_v = 1.
struct SprofWs {
    float* pq;          // [sides][N*C][H][2Wh]: [P | Q] in the forward, [T1 | T2] in the backward
    float* pw;          // [sides][N*C][H][Wh]: the weighted power plane
    float* coef;        // [N*C][K]: the profile op's backward forms its coefficient table here
    long total;
};

static SprofWs sprof_ws(float* ws, long sides, long imgs, long H, long Wh, long K) {
    SprofWs p;
    long off = 0;
    p.pq = ws + off;
    off += sides * imgs * H * 2 * Wh;
    p.pw = ws + off;
    off += sides * imgs * H * Wh;
    p.coef = ws + off;
    off += imgs * K;
    p.total = off;
    return p;
}

// number of radial bins, in integers: 1 + the largest k with k^2 H^2 W^2 <= M^2 ((H/2)^2 W^2 + (W/2)^2 H^2); sides <= 1024 fit int64
static int sprof_bins(long H, long W) {
    const long M = H < W ? H : W, hh = H / 2, ww = W / 2;
    const long num = M * M * (hh * hh * W * W + ww * ww * H * H), den = H * H * W * W;
    long k = 0;
    while ((k + 1) * (k + 1) * den <= num) ++k;
    return (int)k + 1;
}

__device__ __forceinline__ float sprof_mv(int v, int W, int Wh) { return (Wh == W || v == 0 || 2 * v == W) ? 1.f : 2.f; }

// column pass on the half plane for S images (x, or x and y) of one (sample, channel): pw for every image; Re, J only for an image
// whose save pointer is not null (its gradient will be wanted)
template <int S>
__global__ __launch_bounds__(256) void sprof_col_fwd_kernel(const float* __restrict__ pq, const float* __restrict__ tabH,
                                                            float* __restrict__ pw, float* __restrict__ save_x, float* __restrict__ save_y,
                                                            int H, int W, int Wh, long imgs) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[2 * S][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int u0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const float* pqx = pq + img * H * 2 * Wh;
    const float* pqy = pq + (imgs + img) * H * 2 * Wh;
    f32x16 rx, jx, ry, jy;
#pragma unroll
    for (int r = 0; r < 16; ++r) rx[r] = jx[r] = ry[r] = jy[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, u0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int k = k0 + (e >> 6), v = v0 + (e & 63);
            const bool ok = k < H && v < Wh;
            const long o = (long)k * 2 * Wh + v;
            Bs[0][e] = ok ? pqx[o] : 0.f;
            Bs[1][e] = ok ? pqx[o + Wh] : 0.f;
            if (S == 2) {
                Bs[2 * S - 2][e] = ok ? pqy[o] : 0.f;
                Bs[2 * S - 1][e] = ok ? pqy[o + Wh] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float px = Bs[0][bo], qx = Bs[1][bo];
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, px, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(as, px, jx, 0, 0, 0);
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qx, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qx, jx, 0, 0, 0);
            if (S == 2) {
                const float py = Bs[2 * S - 2][bo], qy = Bs[2 * S - 1][bo];
                ry = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, py, ry, 0, 0, 0);
                jy = __builtin_amdgcn_mfma_f32_32x32x2f32(as, py, jy, 0, 0, 0);
                ry = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qy, ry, 0, 0, 0);
                jy = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qy, jy, 0, 0, 0);
            }
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        const long hwh = (long)H * Wh;
        const float mv = sprof_mv(v, W, Wh), hw = (float)(H * W);
        float* pwx = pw + img * hwh;
        float* pwy = pw + (imgs + img) * hwh;
        float* sx = save_x ? save_x + img * 2 * hwh : nullptr;
        float* sy = (S == 2 && save_y) ? save_y + img * 2 * hwh : nullptr;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int u = u0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (u < H) {
                const long o = (long)u * Wh + v;
                pwx[o] = mv * ((rx[rr] * rx[rr] + jx[rr] * jx[rr]) / hw);
                if (sx) {
                    sx[o] = rx[rr];
                    sx[hwh + o] = jx[rr];
                }
                if (S == 2) {
                    pwy[o] = mv * ((ry[rr] * ry[rr] + jy[rr] * jy[rr]) / hw);
                    if (sy) {
                        sy[o] = ry[rr];
                        sy[hwh + o] = jy[rr];
                    }
                }
            }
        }
    }
}

// one wave per (plane, bin): the bin's segment of the CSR list (half-plane indices in ascending order) added lane-strided in double,
// then one butterfly.  A[plane][k] = sum / cnt_k
__global__ __launch_bounds__(256) void sprof_bin_kernel(const float* __restrict__ pw, const int* __restrict__ csr_off,
                                                        const int* __restrict__ csr_idx, const int* __restrict__ cnt, float* __restrict__ A,
                                                        long planes, int K, long hwh) {
    const int lane = threadIdx.x & 63;
    const long id = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= planes * K) return;                           // uniform over the wave
    const int k = (int)(id % K);
    const float* pl = pw + (id / K) * hwh;
    int b = csr_off[k], e = csr_off[k + 1];
    b = b < 0 ? 0 : b;
    e = e > hwh ? (int)hwh : e;
    double s = 0.0;
    for (int i = b + lane; i < e; i += 64) {
        const int j = csr_idx[i];
        if (j >= 0 && j < hwh) s += (double)pl[j];
    }
    s = wave_sum(s);
    if (lane == 0) A[id] = (float)(s / (double)cnt[k]);
}

// dL/dA / cnt_k of one entry, given d = dL/da already scaled
__device__ __forceinline__ float sprof_coef(double d, double A, double eps, int cnt) { return (float)(d / (A + eps) / (double)cnt); }

// single block, double, fixed order.  A: [2][imgs][K].  Paired form: per sample n the sum of (a_x - a_y)^2 over c and k >= k_min by
// the block tree, the samples added in index order.  Batch form: thread k adds a[., k] over the planes in index order, then the
// squared differences of the means go through the tree.  coef_x / coef_y (each may be nullptr) get dL/dA / cnt_k with the mean's
// divisor folded in; per_image: of that sample's own mean
__global__ __launch_bounds__(256) void sprof_finish_kernel(const float* __restrict__ A, const int* __restrict__ cnt, float* __restrict__ loss,
                                                           float* __restrict__ per, float* __restrict__ coef_x, float* __restrict__ coef_y,
                                                           int N, int C, int K, int k_min, double eps, int batch, int per_image) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long imgs = (long)N * C;
    const float* Ax = A;
    const float* Ay = A + imgs * K;
    const double bins = (double)(K - k_min);
    if (batch) {
        double acc = 0.0;
        const double div = bins * (double)imgs;
        for (int k = tid; k < K; k += 256) {
            double sx = 0.0, sy = 0.0;
            for (long p = 0; p < imgs; ++p) {
                sx += log((double)Ax[p * K + k] + eps);
                sy += log((double)Ay[p * K + k] + eps);
            }
            const double d = sx / (double)imgs - sy / (double)imgs;
            const bool in = k >= k_min;
            if (in) acc += d * d;
            const double gx = in ? 2.0 * d / div : 0.0;
            for (long p = 0; p < imgs; ++p) {
                if (coef_x) coef_x[p * K + k] = sprof_coef(gx, (double)Ax[p * K + k], eps, cnt[k]);
                if (coef_y) coef_y[p * K + k] = sprof_coef(-gx, (double)Ay[p * K + k], eps, cnt[k]);
            }
        }
        acc = block_tree_256(acc, red);
        if (tid == 0) *loss = (float)(acc / bins);
        return;
    }
    const double div = (per_image ? 1.0 : (double)N) * (double)C * bins;
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        for (long e = tid; e < (long)C * K; e += 256) {
            const int k = (int)(e % K);
            const long o = ((long)n * C + e / K) * K + k;
            const double ax = (double)Ax[o], ay = (double)Ay[o];
            const double d = log(ax + eps) - log(ay + eps);
            const bool in = k >= k_min;
            if (in) acc += d * d;
            const double gx = in ? 2.0 * d / div : 0.0;
            if (coef_x) coef_x[o] = sprof_coef(gx, ax, eps, cnt[k]);
            if (coef_y) coef_y[o] = sprof_coef(-gx, ay, eps, cnt[k]);
        }
        acc = block_tree_256(acc, red);
        total += acc;
        if (tid == 0 && per) per[n] = (float)(acc / ((double)C * bins));
    }
    if (tid == 0) *loss = (float)(total / ((double)N * (double)C * bins));
}

// the profile op's backward: coef[p][k] = gA[p][k] / cnt_k
__global__ __launch_bounds__(256) void sprof_cotangent_kernel(const float* __restrict__ gA, const int* __restrict__ cnt,
                                                              float* __restrict__ coef, long n, int K) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) coef[i] = gA[i] / (float)cnt[i % K];
}

// [T1 | T2] = [C_H dRe + S_H dJ | C_H dJ - S_H dRe] on the half plane, for the x image (want_x) and / or the y image (want_y);
// (dRe, dJ) = g (2/(HW)) m_v coef[p][bin(u,v)] (Re, J) formed from the saved planes while they are staged.  g: one device scalar,
// or one per sample (g_stride 1), or nullptr (= 1: the profile op, whose cotangent is the coefficient table)
__global__ __launch_bounds__(256) void sprof_col_bwd_kernel(const float* __restrict__ save_x, const float* __restrict__ save_y,
                                                            const float* __restrict__ coef_x, const float* __restrict__ coef_y,
                                                            const short* __restrict__ binmap, const float* __restrict__ tabH,
                                                            const float* __restrict__ g, int g_stride, float* __restrict__ T, int H, int W,
                                                            int Wh, int C, int K, long imgs, float c2, int want_x, int want_y) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int h0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const long hwh = (long)H * Wh;
    const float* plx = want_x ? save_x + img * 2 * hwh : nullptr;
    const float* ply = want_y ? save_y + img * 2 * hwh : nullptr;
    const float* cx = want_x ? coef_x + img * K : nullptr;
    const float* cy = want_y ? coef_y + img * K : nullptr;
    const int sv = v0 + (tid & 63);
    const float gs = (g ? g[(img / C) * g_stride] : 1.f) * c2 * sprof_mv(sv, W, Wh);
    f32x16 t1x, t2x, t1y, t2y;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1x[r] = t2x[r] = t1y[r] = t2y[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, h0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int u = k0 + (e >> 6);
            float drx = 0.f, djx = 0.f, dry = 0.f, djy = 0.f;
            if (u < H && sv < Wh) {
                const long o = (long)u * Wh + sv;
                int b = binmap[o];
                b = b < 0 ? 0 : (b < K ? b : K - 1);
                if (want_x) {
                    const float w = gs * cx[b];
                    drx = w * plx[o];
                    djx = w * plx[hwh + o];
                }
                if (want_y) {
                    const float w = gs * cy[b];
                    dry = w * ply[o];
                    djy = w * ply[hwh + o];
                }
            }
            Bs[0][e] = drx;
            Bs[1][e] = djx;
            Bs[2][e] = dry;
            Bs[3][e] = djy;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            if (want_x) {
                const float dr = Bs[0][bo], dj = Bs[1][bo];
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2x, 0, 0, 0);
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2x, 0, 0, 0);
            }
            if (want_y) {
                const float dr = Bs[2][bo], dj = Bs[3][bo];
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2y, 0, 0, 0);
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2y, 0, 0, 0);
            }
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        float* Tx = T + img * H * 2 * Wh;
        float* Ty = T + (imgs + img) * H * 2 * Wh;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = h0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (h < H) {
                const long o = (long)h * 2 * Wh + v;
                if (want_x) {
                    Tx[o] = t1x[rr];
                    Tx[o + Wh] = t2x[rr];
                }
                if (want_y) {
                    Ty[o] = t1y[rr];
                    Ty[o + Wh] = t2y[rr];
                }
            }
        }
    }
}

static int sprof_check(const char* what, int sides, int N, int C, int H, int W, int Wh, int K) {
    if (N < 1 || C < 1 || H < 2 || W < 2) return fail(FAOCTASR_EINVAL, "%s: bad shape N %d C %d H %d W %d (H, W >= 2)", what, N, C, H, W);
    if (H > 1024 || W > 1024) return fail(FAOCTASR_EUNSUPPORTED, "%s: H %d, W %d > 1024", what, H, W);
    if ((long)N * C * sides > 65535) return fail(FAOCTASR_EUNSUPPORTED, "%s: %d * N*C %ld > 65535", what, sides, (long)N * C);
    if ((long)N * C * H > (1L << 21)) return fail(FAOCTASR_EUNSUPPORTED, "%s: N*C*H %ld > 2^21", what, (long)N * C * H);
    if (Wh != W / 2 + 1 && Wh != W) return fail(FAOCTASR_EINVAL, "%s: Wh %d is neither W/2 + 1 = %d nor W = %d", what, Wh, W / 2 + 1, W);
    if (K != sprof_bins(H, W)) return fail(FAOCTASR_EINVAL, "%s: K %d, but %d x %d has %d radial bins", what, K, H, W, sprof_bins(H, W));
    return FAOCTASR_OK;
}

// row pass, column pass and binning of `sides` images (y == nullptr: one)
static int sprof_profiles(const char* what, const float* x, const float* y, const float* tabH, const float* halfW, const int* csr_off,
                          const int* csr_idx, const int* cnt, float* A, float* save_x, float* save_y, const SprofWs& p, int N, int C, int H,
                          int W, int Wh, int K, hipStream_t stream) {
    const long imgs = (long)N * C;
    const int sides = y ? 2 : 1;
    long diff = 0;
    if (y) {
        const intptr_t d = (intptr_t)y - (intptr_t)x;
        if (d % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "%s: x and y are not 4-byte aligned to each other", what);
        diff = (long)(d / (intptr_t)sizeof(float));
    }
    int rc = faoctasr_sgemm_batched(x, halfW, p.pq, (int)(imgs * H), 2 * Wh, W, W, 2 * Wh, 2 * Wh, diff, 0, imgs * H * 2 * Wh, sides,
                                    (faoctasr_stream_t)stream);
    if (rc) return rc;
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    if (y)
        hipLaunchKernelGGL(sprof_col_fwd_kernel<2>, grid, dim3(256), 0, stream, (const float*)p.pq, tabH, p.pw, save_x, save_y, H, W, Wh, imgs);
    else
        hipLaunchKernelGGL(sprof_col_fwd_kernel<1>, grid, dim3(256), 0, stream, (const float*)p.pq, tabH, p.pw, save_x, save_y, H, W, Wh, imgs);
    rc = check_launch(what);
    if (rc) return rc;
    const long waves = sides * imgs * K;
    hipLaunchKernelGGL(sprof_bin_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, (const float*)p.pw, csr_off, csr_idx, cnt, A,
                       sides * imgs, K, (long)H * Wh);
    return check_launch(what);
}

// ---- Fourier ring correlation (Saxton & Baumeister 1982; van Heel & Schatz 2005) --------------------------------------------------
//   F = fft2(x), G = fft2(y);  per plane and ring k of the spectral profile's geometry, the ring MEANS
//   Nk = mean Re(F conj G) / (HW),  Xk = mean |F|^2 / (HW),  Yk = mean |G|^2 / (HW)      (Xk, Yk: the spectral profiles, bit for bit)
//   r_k = Nk / sqrt(Xk Yk + eps)  in double;  index = mean of r_k over c and k_min <= k <= k_max;  curve = r_k at every ring
// The spectral profile's path with both transforms kept complex and three ring sums in place of one:
//   [P | Q] = X [C_W[:, :Wh] | S_W[:, :Wh]]        row pass, x and y in one launch
//   Re, J of both images on H x Wh;  three weighted half planes m_v (Rx Ry + Jx Jy)/HW, m_v |F|^2/HW, m_v |G|^2/HW from the accumulators
//   one sprof_bin_kernel launch over the 3 N*C planes;  finish (one block, double, fixed order): curve, index, coefficient tables
//   backward: (dRe_x, dJ_x) = g m_v/(HW) (cN[bin] (Re_y, J_y) + 2 cX[bin] (Re_x, J_x)), the mirror image for y, formed while staging;
//   [T1 | T2] as above;  dX = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]
// A ring with Xk Yk = 0 has Nk = 0 (Cauchy-Schwarz, term by term): r_k = 0 and every coefficient is finite (D = sqrt(eps)).
// x and y run one instruction sequence each: frc(x, y) == frc(y, x) bit for bit, with swapped gradients.
struct FrcWs {
    float* pq;          // [2 (x,y)][N*C][H][2Wh]: [P | Q] in the forward, [T1 | T2] in the backward
    float* pw;          // [3 (N,X,Y)][N*C][H][Wh]: the weighted half planes
    long total;
};

static FrcWs frc_ws(float* ws, long imgs, long H, long Wh) {
    FrcWs p;
    long off = 0;
    p.pq = ws + off;
    off += 2 * imgs * H * 2 * Wh;
    p.pw = ws + off;
    off += 3 * imgs * H * Wh;
    p.total = off;
    return p;
}

// column pass of sprof_col_fwd_kernel<2>; the epilogue writes the cross plane and both power planes, and with `save` Re, J of BOTH
// images ([2 (x,y)][N*C][2 (Re,J)][H][Wh]): the gradient of either image reads the other's spectrum
__global__ __launch_bounds__(256) void frc_col_fwd_kernel(const float* __restrict__ pq, const float* __restrict__ tabH,
                                                          float* __restrict__ pw, float* __restrict__ save, int H, int W, int Wh, long imgs) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int u0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const float* pqx = pq + img * H * 2 * Wh;
    const float* pqy = pq + (imgs + img) * H * 2 * Wh;
    f32x16 rx, jx, ry, jy;
#pragma unroll
    for (int r = 0; r < 16; ++r) rx[r] = jx[r] = ry[r] = jy[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, u0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int k = k0 + (e >> 6), v = v0 + (e & 63);
            const bool ok = k < H && v < Wh;
            const long o = (long)k * 2 * Wh + v;
            Bs[0][e] = ok ? pqx[o] : 0.f;
            Bs[1][e] = ok ? pqx[o + Wh] : 0.f;
            Bs[2][e] = ok ? pqy[o] : 0.f;
            Bs[3][e] = ok ? pqy[o + Wh] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float px = Bs[0][bo], qx = Bs[1][bo];
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, px, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(as, px, jx, 0, 0, 0);
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qx, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qx, jx, 0, 0, 0);
            const float py = Bs[2][bo], qy = Bs[3][bo];
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, py, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(as, py, jy, 0, 0, 0);
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qy, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qy, jy, 0, 0, 0);
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        const long hwh = (long)H * Wh;
        const float mv = sprof_mv(v, W, Wh), hw = (float)(H * W);
        float* pwn = pw + img * hwh;
        float* pwx = pw + (imgs + img) * hwh;
        float* pwy = pw + (2 * imgs + img) * hwh;
        float* sx = save ? save + img * 2 * hwh : nullptr;
        float* sy = save ? save + (imgs + img) * 2 * hwh : nullptr;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int u = u0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (u < H) {
                const long o = (long)u * Wh + v;
                pwn[o] = mv * ((rx[rr] * ry[rr] + jx[rr] * jy[rr]) / hw);
                pwx[o] = mv * ((rx[rr] * rx[rr] + jx[rr] * jx[rr]) / hw);
                pwy[o] = mv * ((ry[rr] * ry[rr] + jy[rr] * jy[rr]) / hw);
                if (save) {
                    sx[o] = rx[rr];
                    sx[hwh + o] = jx[rr];
                    sy[o] = ry[rr];
                    sy[hwh + o] = jy[rr];
                }
            }
        }
    }
}

// single block, double, fixed order.  A: [3 (N,X,Y)][imgs][K] ring means.  Per sample n the sum of r over c and k_min <= k <= k_max
// by the block tree, the samples added in index order.  coef ([3 (cN,cX,cY)][imgs][K], may be nullptr): d index / d (Nk, Xk, Yk)
// over cnt_k with the mean's divisor folded in (per_image: that sample's own mean), zero outside the band
__global__ __launch_bounds__(256) void frc_finish_kernel(const float* __restrict__ A, const int* __restrict__ cnt, float* __restrict__ index,
                                                         float* __restrict__ per, float* __restrict__ curve, float* __restrict__ coef, int N,
                                                         int C, int K, int k_min, int k_max, double eps, int per_image) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long imgs = (long)N * C;
    const float* An = A;
    const float* Ax = A + imgs * K;
    const float* Ay = A + 2 * imgs * K;
    const double rings = (double)(k_max - k_min + 1);
    const double w = 1.0 / ((per_image ? 1.0 : (double)N) * (double)C * rings);
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        for (long e = tid; e < (long)C * K; e += 256) {
            const int k = (int)(e % K);
            const long o = ((long)n * C + e / K) * K + k;
            const double nk = (double)An[o], xk = (double)Ax[o], yk = (double)Ay[o];
            const double D = sqrt(xk * yk + eps);
            const double r = nk / D;
            const bool in = k >= k_min && k <= k_max;
            curve[o] = (float)r;
            if (in) acc += r;
            if (coef) {
                const double c = (double)cnt[k], d3 = 2.0 * (D * D * D);
                coef[o] = in ? (float)(w / D / c) : 0.f;
                coef[imgs * K + o] = in ? (float)(-(w * nk * yk) / d3 / c) : 0.f;
                coef[2 * imgs * K + o] = in ? (float)(-(w * nk * xk) / d3 / c) : 0.f;
            }
        }
        acc = block_tree_256(acc, red);
        total += acc;
        if (tid == 0 && per) per[n] = (float)(acc / ((double)C * rings));
    }
    if (tid == 0) *index = (float)(total / ((double)N * (double)C * rings));
}

// sprof_col_bwd_kernel's transform; the operand of a side is formed from BOTH saved images while they are staged:
// (dRe_x, dJ_x) = g m_v/(HW) (cN[bin] (Re_y, J_y) + 2 cX[bin] (Re_x, J_x)), and with x and y exchanged for y.  g: one device scalar, or
// one per sample (g_stride 1).  A side that is not wanted costs neither operand, MFMA chain nor stores
__global__ __launch_bounds__(256) void frc_col_bwd_kernel(const float* __restrict__ save, const float* __restrict__ coef,
                                                          const short* __restrict__ binmap, const float* __restrict__ tabH,
                                                          const float* __restrict__ g, int g_stride, float* __restrict__ T, int H, int W, int Wh,
                                                          int C, int K, long imgs, float c1, int want_x, int want_y) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int h0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const long hwh = (long)H * Wh;
    const float* plx = save + img * 2 * hwh;
    const float* ply = save + (imgs + img) * 2 * hwh;
    const float* cn = coef + img * K;
    const float* cx = coef + (imgs + img) * K;
    const float* cy = coef + (2 * imgs + img) * K;
    const int sv = v0 + (tid & 63);
    const float gs = g[(img / C) * g_stride] * c1 * sprof_mv(sv, W, Wh);
    f32x16 t1x, t2x, t1y, t2y;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1x[r] = t2x[r] = t1y[r] = t2y[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, h0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int u = k0 + (e >> 6);
            float drx = 0.f, djx = 0.f, dry = 0.f, djy = 0.f;
            if (u < H && sv < Wh) {
                const long o = (long)u * Wh + sv;
                int b = binmap[o];
                b = b < 0 ? 0 : (b < K ? b : K - 1);
                const float rex = plx[o], imx = plx[hwh + o], rey = ply[o], imy = ply[hwh + o];
                const float kn = cn[b];
                if (want_x) {
                    const float ks = 2.f * cx[b];
                    drx = gs * (kn * rey + ks * rex);
                    djx = gs * (kn * imy + ks * imx);
                }
                if (want_y) {
                    const float ks = 2.f * cy[b];
                    dry = gs * (kn * rex + ks * rey);
                    djy = gs * (kn * imx + ks * imy);
                }
            }
            Bs[0][e] = drx;
            Bs[1][e] = djx;
            Bs[2][e] = dry;
            Bs[3][e] = djy;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            if (want_x) {
                const float dr = Bs[0][bo], dj = Bs[1][bo];
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2x, 0, 0, 0);
                t1x = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1x, 0, 0, 0);
                t2x = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2x, 0, 0, 0);
            }
            if (want_y) {
                const float dr = Bs[2][bo], dj = Bs[3][bo];
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dr, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, dj, t2y, 0, 0, 0);
                t1y = __builtin_amdgcn_mfma_f32_32x32x2f32(as, dj, t1y, 0, 0, 0);
                t2y = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, dr, t2y, 0, 0, 0);
            }
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        float* Tx = T + img * H * 2 * Wh;
        float* Ty = T + (imgs + img) * H * 2 * Wh;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = h0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (h < H) {
                const long o = (long)h * 2 * Wh + v;
                if (want_x) {
                    Tx[o] = t1x[rr];
                    Tx[o + Wh] = t2x[rr];
                }
                if (want_y) {
                    Ty[o] = t1y[rr];
                    Ty[o + Wh] = t2y[rr];
                }
            }
        }
    }
}

// ---- phase-correlation registration and the Fourier shift (Kuglin & Hines 1975; Guizar-Sicairos, Thurman & Fienup 2008) ----------
//   F = fft2(a), G = fft2(b);  R = G conj(F) / (HW),  Rn = R / sqrt(|R|^2 + eps) (or R), zero in every ring above k_max
//   surface = sum_c Re ifft2(Rn): its peak lies at d when b(p) = a(p - d);  the coarse peak is the first maximum inside the window
//   up[j,i] = (1/HW) sum_c sum_u sum_{v<Wh} m_v Re(Rn[c,u,v] exp(2 pi i (f_u (s_y + o_j) + f_v (s_x + o_i)))),  o_j = (j - T/2) / U:
//   the inverse transform evaluated on T x T points around the coarse peak, as two small DFT-as-GEMM contractions
// The FRC forward with an epilogue that keeps only Rn, and the first forward use of the half-spectrum inverse, which so far existed
// as backward passes: with a half plane Z = A - iB (the convention of Re, J above) of a real image,
//   [T1 | T2] = [C_H A + S_H B | C_H B - S_H A]  on the operand m_v/(HW) Z;   X = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]
// hspec_inv_col_kernel is that column pass.  Its table is either the H-point DFT table or a per-sample T x H table of the upsampled
// DFT, so the refinement's first contraction is the same kernel; its operand is summed over the channels while it is staged (the
// surface and `up` are sums over c of a linear map), or multiplied by the ramp of the Fourier shift
//   fourier_shift(x, d) = Re ifft2(fft2(x) exp(-2 pi i (f_u d_y + f_v d_x))),  f of numpy.fft.fftfreq (Nyquist at -1/2):
// the real part turns the Nyquist row and column (even sides) into cos(pi d_y), cos(pi d_x) and the bin that is Nyquist on both axes
// into cos(pi (d_y + d_x)): the effective ramp is Hermitian, and separable everywhere but in that one bin.
// No atomics; every sum in a fixed order; nothing here waits for the host: the peak stays on the device between the launches.
struct PcorrWs {
    float* pq;          // [2 (a,b)][N*C][H][2Wh]: [P | Q]; then [N][H][2Wh]: [T1 | T2] of the inverse
    float* rn;          // [N*C][2][H][Wh]: Rn as (Re, -Im)
    float* surf;        // [N][H][W] when the caller does not ask for the surface
    float* ey;          // [N][H][2T]: cos | sin of 2 pi f_u (s_y + o_j)
    float* ex;          // [N][2][Wh][T]: cos, sin of 2 pi f_v (s_x + o_i)
    float* up;          // [N][T][2Wh]: [T1 | T2] of the refinement
    int* coarse;        // [N][2]: the coarse peak (s_y, s_x), signed
    long total;
};

static int pcorr_points(int U) { return (3 * U + 1) / 2; }              // T = ceil(1.5 U)

static PcorrWs pcorr_ws(float* ws, long N, long C, long H, long W, long Wh, long U) {
    PcorrWs p;
    const long T = U > 1 ? pcorr_points((int)U) : 0;
    long off = 0;
    p.pq = ws + off;
    off += 2 * N * C * H * 2 * Wh;
    p.rn = ws + off;
    off += N * C * 2 * H * Wh;
    p.surf = ws + off;
    off += N * H * W;
    p.ey = ws + off;
    off += N * H * 2 * T;
    p.ex = ws + off;
    off += N * 2 * Wh * T;
    p.up = ws + off;
    off += N * T * 2 * Wh;
    p.coarse = (int*)(ws + off);
    off += 2 * N;
    p.total = off;
    return p;
}

struct FshiftWs {
    float* pq;          // [N*C][H][2Wh]: [P | Q] in the forward passes, [T1 | T2] in the inverse ones
    float* planes;      // [N*C][2][H][Wh]: Re, -Im
    float* pw;          // [N*C][H][Wh]: the power plane sprof_col_fwd_kernel also writes (not read)
    long total;
};

static FshiftWs fshift_ws(float* ws, long imgs, long H, long Wh) {
    FshiftWs p;
    long off = 0;
    p.pq = ws + off;
    off += imgs * H * 2 * Wh;
    p.planes = ws + off;
    off += imgs * 2 * H * Wh;
    p.pw = ws + off;
    off += imgs * H * Wh;
    p.total = off;
    return p;
}

// every product of the two spectra in one place: G conj(F) for F = rx - i jx, G = ry - i jy, as (Re, -Im).  Exchanging the images
// leaves re and negates im exactly (the caller compiles this without contraction)
__device__ __forceinline__ void pcorr_cross(float rx, float jx, float ry, float jy, float& re, float& im) {
#pragma clang fp contract(off)
    re = rx * ry + jx * jy;
    im = jy * rx - ry * jx;
}

// column pass of frc_col_fwd_kernel; the epilogue forms Rn from the four accumulators and writes that half plane only
__global__ __launch_bounds__(256) void pcorr_col_fwd_kernel(const float* __restrict__ pq, const float* __restrict__ tabH,
                                                            const short* __restrict__ binmap, float* __restrict__ rn, int H, int W, int Wh,
                                                            long imgs, float eps, int k_max, int normalize) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[4][PH_KC * PH_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long img = blockIdx.z;
    const int u0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const float* pqx = pq + img * H * 2 * Wh;
    const float* pqy = pq + (imgs + img) * H * 2 * Wh;
    f32x16 rx, jx, ry, jy;
#pragma unroll
    for (int r = 0; r < 16; ++r) rx[r] = jx[r] = ry[r] = jy[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables(Cs, Ss, tabH, H, k0, u0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int k = k0 + (e >> 6), v = v0 + (e & 63);
            const bool ok = k < H && v < Wh;
            const long o = (long)k * 2 * Wh + v;
            Bs[0][e] = ok ? pqx[o] : 0.f;
            Bs[1][e] = ok ? pqx[o + Wh] : 0.f;
            Bs[2][e] = ok ? pqy[o] : 0.f;
            Bs[3][e] = ok ? pqy[o + Wh] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float px = Bs[0][bo], qx = Bs[1][bo];
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, px, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(as, px, jx, 0, 0, 0);
            rx = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qx, rx, 0, 0, 0);
            jx = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qx, jx, 0, 0, 0);
            const float py = Bs[2][bo], qy = Bs[3][bo];
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, py, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(as, py, jy, 0, 0, 0);
            ry = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, qy, ry, 0, 0, 0);
            jy = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, qy, jy, 0, 0, 0);
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        const long hwh = (long)H * Wh;
        const float hw = (float)(H * W);
        float* out = rn + img * 2 * hwh;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int u = u0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (u < H) {
                const long o = (long)u * Wh + v;
                float re, im;
                pcorr_cross(rx[rr], jx[rr], ry[rr], jy[rr], re, im);
                re = re / hw;
                im = im / hw;
                if (normalize) {
                    const float d = sqrtf(re * re + im * im + eps);
                    re = re / d;
                    im = im / d;
                }
                if (binmap[o] > k_max) re = im = 0.f;
                out[o] = re;
                out[hwh + o] = im;
            }
        }
    }
}

// stage one 16 x 64 chunk of a table pair stored k-major: C[k][r] at tab[k * ld + r], S[k][r] at tab[k * ld + half + r], k < K, r < R
__device__ __forceinline__ void stage_tables_ld(float* Cs, float* Ss, const float* __restrict__ tab, int K, int R, int ld, int half, int k0,
                                                int r0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = tid + 256 * i;
        const int k = k0 + (e >> 6), r = r0 + (e & 63);
        const bool ok = k < K && r < R;
        Cs[e] = ok ? tab[(long)k * ld + r] : 0.f;
        Ss[e] = ok ? tab[(long)k * ld + half + r] : 0.f;
    }
}

// (cos, sin) of 2 pi (k / n) d for the signed index k of a ramp; the phase is reduced in double before sincospi.  The Nyquist index
// of an even side gives (cos(pi d), 0): the real part of the shifted image (see above; the caller treats the doubly-Nyquist bin)
__device__ __forceinline__ void shift_ramp(int idx, int n, float d, float& c, float& s) {
    const int k = centred(idx, n);
    double t = (double)k * (double)d / (double)n;
    t -= rint(t);
    double sd, cd;
    sincospi(2.0 * t, &sd, &cd);
    c = (float)cd;
    s = (2 * idx == n) ? 0.f : (float)sd;
}

// the half-spectrum inverse column pass: T[out][r][0..2Wh) = [T1 | T2], T1 = sum_u C[u][r] A' + S[u][r] B', T2 = sum_u C[u][r] B' - S[u][r] A',
// r < R, for the table pair `tab` (+ n * tab_stride: per sample, or 0), k-major with row length ld = 2R.  The operand (A', B') is formed
// from planes[img][2][H][Wh] while it is staged: csum: the sum over the C channels of sample n = out (in index order), else the plane
// out with n = out / C;  then, with `shift`, times the ramp of fourier_shift for d = sign * shift[n];  then times m_v * scale.
// scale is 1 / (HW) for the Fourier shift.  Phase correlation passes 1 and divides once behind the last sum: where Rn is 1 in every
// bin (an image against itself) the operands are then small integers, every sum is exact and the peak is exactly 1
__global__ __launch_bounds__(256) void hspec_inv_col_kernel(const float* __restrict__ planes, const float* __restrict__ tab, long tab_stride,
                                                            int R, int ld, const float* __restrict__ shift, float sign, float scale,
                                                            float* __restrict__ T, int H, int W, int Wh, int C, int csum) {
#pragma clang fp contract(off)
    __shared__ float Cs[PH_KC * PH_T], Ss[PH_KC * PH_T], Bs[2][PH_KC * PH_T];
    __shared__ float gyc[1024], gys[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long out = blockIdx.z;
    const long n = csum ? out : out / C;
    const int r0 = blockIdx.y * PH_T, v0 = blockIdx.x * PH_T;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const long hwh = (long)H * Wh;
    const float* pl = planes + (csum ? out * C : out) * 2 * hwh;
    const int cn = csum ? C : 1;
    const float* tb = tab + n * tab_stride;
    const int sv = v0 + (tid & 63);
    const float wv = sprof_mv(sv, W, Wh) * scale;
    float gxc = 1.f, gxs = 0.f, gnn = 1.f;
    if (shift) {
        const float dy = sign * shift[2 * n], dx = sign * shift[2 * n + 1];
        if (sv < Wh) shift_ramp(sv, W, dx, gxc, gxs);
        if (2 * sv == W) {                                      // the bin that is Nyquist on both axes: cos(pi (d_y + d_x))
            double t = 0.5 * ((double)dy + (double)dx);
            t -= rint(t);
            gnn = (float)cospi(2.0 * t);
        }
        for (int u = tid; u < H; u += 256) shift_ramp(u, H, dy, gyc[u], gys[u]);
    }
    f32x16 t1, t2;
#pragma unroll
    for (int r = 0; r < 16; ++r) t1[r] = t2[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += PH_KC) {
        __syncthreads();
        stage_tables_ld(Cs, Ss, tb, H, R, ld, R, k0, r0, tid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int u = k0 + (e >> 6);
            float a = 0.f, b = 0.f;
            if (u < H && sv < Wh) {
                const long o = (long)u * Wh + sv;
                for (int c = 0; c < cn; ++c) {
                    a += pl[c * 2 * hwh + o];
                    b += pl[c * 2 * hwh + hwh + o];
                }
                if (shift) {
                    // g = exp(-i (psi_y + psi_x)) = gr + i gi;  (A - iB) g = (A gr + B gi) - i (B gr - A gi)
                    const float cy = gyc[u], sy = gys[u];
                    const bool nn = 2 * u == H && 2 * sv == W;
                    const float gr = nn ? gnn : cy * gxc - sy * gxs, gi = nn ? 0.f : -(sy * gxc + cy * gxs);
                    const float a2 = a * gr + b * gi, b2 = b * gr - a * gi;
                    a = a2;
                    b = b2;
                }
                a = a * wv;
                b = b * wv;
            }
            Bs[0][e] = a;
            Bs[1][e] = b;
        }
        __syncthreads();
#pragma unroll
        for (int kk0 = 0; kk0 < PH_KC; kk0 += 2) {
            const int ao = (kk0 + lh) * PH_T + wm * 32 + l31, bo = (kk0 + lh) * PH_T + wn * 32 + l31;
            const float ac = Cs[ao], as = Ss[ao], nas = -as;
            const float a = Bs[0][bo], b = Bs[1][bo];
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, a, t1, 0, 0, 0);
            t2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, b, t2, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, b, t1, 0, 0, 0);
            t2 = __builtin_amdgcn_mfma_f32_32x32x2f32(nas, a, t2, 0, 0, 0);
        }
    }
    const int v = v0 + wn * 32 + l31;
    if (v < Wh) {
        float* To = T + out * R * 2 * Wh;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int r = r0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (r < R) {
                const long o = (long)r * 2 * Wh + v;
                To[o] = t1[rr];
                To[o + Wh] = t2[rr];
            }
        }
    }
}

// the better of two (value, index) candidates: the larger value, the lower index on a tie.  A NaN never enters (the caller's
// comparison is false for it), so none is ever held
__device__ __forceinline__ bool peak_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// the block's best candidate by a tree in LDS; valid in thread 0
__device__ __forceinline__ void peak_tree_256(double& v, int& i, double* rv, int* ri) {
    const int tid = threadIdx.x;
    rv[tid] = v;
    ri[tid] = i;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o && peak_better(rv[tid + o], ri[tid + o], rv[tid], ri[tid])) {
            rv[tid] = rv[tid + o];
            ri[tid] = ri[tid + o];
        }
        __syncthreads();
    }
    v = rv[0];
    i = ri[0];
}

// one block per sample: the first maximum of the surface in row-major order among the positions with |d_y| <= my, |d_x| <= mx
// (positions > H/2, > W/2 wrap negative).  The surface comes unscaled (HW times its value).  Writes the signed peak, and shift / peak (the value over C) as they stand without a refinement.
// A plane without a comparable value (all NaN) yields position 0
__global__ __launch_bounds__(256) void pcorr_peak_kernel(const float* __restrict__ surf, int* __restrict__ coarse, float* __restrict__ shift,
                                                         float* __restrict__ peak, int H, int W, int C, int my, int mx) {
    __shared__ double rv[256];
    __shared__ int ri[256];
    const int tid = threadIdx.x, total = H * W;
    const float* s = surf + (long)blockIdx.x * total;
    double best = -INFINITY;
    int idx = 0x7fffffff;
    for (int e = tid; e < total; e += 256) {
        const int y = e / W, x = e % W;
        const int dy = y > H / 2 ? y - H : y, dx = x > W / 2 ? x - W : x;
        if (dy < -my || dy > my || dx < -mx || dx > mx) continue;
        const double v = (double)s[e];
        if (peak_better(v, e, best, idx)) {
            best = v;
            idx = e;
        }
    }
    peak_tree_256(best, idx, rv, ri);
    if (tid == 0) {
        if (idx < 0 || idx >= total) idx = 0;
        const int y = idx / W, x = idx % W;
        const int dy = y > H / 2 ? y - H : y, dx = x > W / 2 ? x - W : x;
        coarse[2 * blockIdx.x] = dy;
        coarse[2 * blockIdx.x + 1] = dx;
        shift[2 * blockIdx.x] = (float)dy;
        shift[2 * blockIdx.x + 1] = (float)dx;
        peak[blockIdx.x] = (float)((double)s[idx] / ((double)H * (double)W * (double)C));
    }
}

// the per-sample tables of the upsampled DFT around the coarse peak, built on the device from it:
//   ey[n][u][j | T + j] = cos | sin of 2 pi u_c (s_y U + j - T/2) / (U H),   ex[n][0 | 1][v][i] likewise for the columns v < Wh.
// The numerator is reduced mod U H (mod U W) in integers before sincospi
__global__ __launch_bounds__(256) void pcorr_twiddle_kernel(const int* __restrict__ coarse, float* __restrict__ ey, float* __restrict__ ex, int H,
                                                            int W, int Wh, int U, int T) {
    const int n = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long ny = (long)H * T, nx = (long)Wh * T;
    if (e >= ny + nx) return;
    const bool isy = e < ny;
    const long e2 = isy ? e : e - ny;
    const int f = (int)(e2 / T), j = (int)(e2 % T);
    const int side = isy ? H : W;
    const long den = (long)U * side;
    long num = ((long)centred(f, side) * ((long)coarse[2 * n + (isy ? 0 : 1)] * U + j - T / 2)) % den;
    if (num < 0) num += den;
    double sd, cd;
    sincospi(2.0 * (double)num / (double)den, &sd, &cd);
    if (isy) {
        float* o = ey + ((long)n * H + f) * 2 * T;
        o[j] = (float)cd;
        o[T + j] = (float)sd;
    } else {
        float* o = ex + (long)n * 2 * nx;
        o[(long)f * T + j] = (float)cd;
        o[nx + (long)f * T + j] = (float)sd;
    }
}

// the surface as the caller sees it: the unscaled sum over HW
__global__ __launch_bounds__(256) void pcorr_scale_kernel(float* __restrict__ surf, long n, float hw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) surf[i] = surf[i] / hw;
}

// one block per sample: up[j][i] = sum_{v<Wh} T1[j][v] cos_x[v][i] + T2[j][v] sin_x[v][i] in double and index order, its first maximum
// in row-major order, and from it shift = (s + (j* - T/2) / U) and peak = up[j*][i*] / (HW C) (the operand came unscaled)
__global__ __launch_bounds__(256) void pcorr_refine_kernel(const float* __restrict__ up, const float* __restrict__ ex, const int* __restrict__ coarse,
                                                           float* __restrict__ shift, float* __restrict__ peak, int Wh, double hwc, int U, int T) {
#pragma clang fp contract(off)
    __shared__ double rv[256];
    __shared__ int ri[256];
    const int tid = threadIdx.x, n = blockIdx.x;
    const float* t = up + (long)n * T * 2 * Wh;
    const float* cx = ex + (long)n * 2 * Wh * T;
    const float* sx = cx + (long)Wh * T;
    double best = -INFINITY;
    int idx = 0x7fffffff;
    for (int e = tid; e < T * T; e += 256) {
        const int j = e / T, i = e % T;
        const float* t1 = t + (long)j * 2 * Wh;
        double acc = 0.0;
        for (int v = 0; v < Wh; ++v) acc += (double)t1[v] * (double)cx[(long)v * T + i] + (double)t1[Wh + v] * (double)sx[(long)v * T + i];
        if (peak_better(acc, e, best, idx)) {
            best = acc;
            idx = e;
        }
    }
    peak_tree_256(best, idx, rv, ri);
    if (tid == 0) {
        if (idx < 0 || idx >= T * T) {                         // no comparable value: the coarse peak stands, the value says why
            idx = (T / 2) * T + T / 2;
            best = NAN;
        }
        const int j = idx / T, i = idx % T;
        shift[2 * n] = (float)((double)(coarse[2 * n] * U + j - T / 2) / (double)U);
        shift[2 * n + 1] = (float)((double)(coarse[2 * n + 1] * U + i - T / 2) / (double)U);
        peak[n] = (float)(best / hwc);
    }
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" int faoctasr_dft_tables(float* out, int n, faoctasr_stream_t stream) {
    if (!out) return fail(FAOCTASR_EINVAL, "dft_tables: null pointer");
    if (n < 1 || n > 8192) return fail(FAOCTASR_EINVAL, "dft_tables: n %d outside [1, 8192]", n);
    const long total = (long)n * n;
    hipLaunchKernelGGL(dft_tables_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n);
    return check_launch("dft_tables");
}

extern "C" long faoctasr_phase_loss_workspace_floats(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 2 || W < 2) {
        fail(FAOCTASR_EINVAL, "phase_loss_workspace_floats: bad shape N %d C %d H %d W %d (H, W >= 2)", N, C, H, W);
        return -1;
    }
    return phase_ws(nullptr, N, C, H, W).total;
}

extern "C" int faoctasr_phase_loss_fwd(const float* x, const float* y, const float* tabH, const float* tabW, float radius,
                                       float* loss_per_sample, float* loss_mean, float* workspace, int N, int C, int H, int W,
                                       faoctasr_stream_t stream) {
    if (!x || !y || !tabH || !tabW || !loss_per_sample || !loss_mean || !workspace) return fail(FAOCTASR_EINVAL, "phase_loss_fwd: null pointer");
    int rc = phase_check("phase_loss_fwd", workspace, N, C, H, W, radius);
    if (rc) return rc;
    const PhaseWs p = phase_ws(workspace, N, C, H, W);
    const long imgs = (long)N * C;
    // row pass [P | Q] = X [C_W | S_W]: x and y as the two batch entries of one launch (the stride is their address difference)
    const intptr_t diff = (intptr_t)y - (intptr_t)x;
    if (diff % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "phase_loss_fwd: x and y are not 4-byte aligned to each other");
    rc = faoctasr_sgemm_batched(x, tabW, p.pq, (int)(imgs * H), 2 * W, W, W, 2 * W, 2 * W, (long)(diff / (intptr_t)sizeof(float)), 0,
                                imgs * H * 2 * W, 2, stream);
    if (rc) return rc;
    const double inv2r2 = 0.5 / ((double)radius * (double)radius);
    dim3 grid((W + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(phase_col_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p.pq, tabH, p.planes, p.part, H, W, imgs,
                       inv2r2);
    rc = check_launch("phase_loss_fwd (column pass)");
    if (rc) return rc;
    hipLaunchKernelGGL(phase_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)p.part, p.stats, loss_per_sample,
                       loss_mean, N, (long)C * grid.x * grid.y);
    return check_launch("phase_loss_fwd (finish)");
}

extern "C" int faoctasr_phase_loss_bwd(const float* g, const float* tabH, const float* tabW, float radius, float* dx, float* dy,
                                       float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream) {
    if (!g || !tabH || !tabW || !workspace) return fail(FAOCTASR_EINVAL, "phase_loss_bwd: null pointer");
    int rc = phase_check("phase_loss_bwd", workspace, N, C, H, W, radius);
    if (rc) return rc;
    if (!dx && !dy) return FAOCTASR_OK;
    const PhaseWs p = phase_ws(workspace, N, C, H, W);
    const long imgs = (long)N * C;
    const double inv2r2 = 0.5 / ((double)radius * (double)radius);
    dim3 grid((W + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(phase_col_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p.planes, tabH, (const double*)p.stats, g,
                       p.pq, H, W, C, N, imgs, inv2r2, dx ? 1 : 0, dy ? 1 : 0);
    rc = check_launch("phase_loss_bwd (column pass)");
    if (rc) return rc;
    // dX = [T1 | T2] [C_W ; S_W]: the stacked table is the second half of the table buffer
    const float* stacked = tabW + 2L * W * W;
    const long sT = imgs * H * 2 * W;
    if (dx && dy) {
        const intptr_t diff = (intptr_t)dy - (intptr_t)dx;
        if (diff % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "phase_loss_bwd: dx and dy are not 4-byte aligned to each other");
        return faoctasr_sgemm_batched(p.pq, stacked, dx, (int)(imgs * H), W, 2 * W, 2 * W, W, W, sT, 0, (long)(diff / (intptr_t)sizeof(float)), 2,
                                      stream);
    }
    return faoctasr_sgemm_batched(dx ? p.pq : p.pq + sT, stacked, dx ? dx : dy, (int)(imgs * H), W, 2 * W, 2 * W, W, W, 0, 0, 0, 1, stream);
}

extern "C" long faoctasr_ffl_workspace_floats(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 2 || W < 2) {
        fail(FAOCTASR_EINVAL, "ffl_workspace_floats: bad shape N %d C %d H %d W %d (H, W >= 2)", N, C, H, W);
        return -1;
    }
    return ffl_ws(nullptr, N, C, H, W).total;
}

extern "C" int faoctasr_ffl_fwd(const float* x, const float* y, const float* tabH, const float* tabW, float alpha, int log_matrix,
                                int batch_matrix, float* loss, float* planes, float* workspace, int N, int C, int H, int W,
                                faoctasr_stream_t stream) {
    if (!x || !y || !tabH || !tabW || !loss || !workspace) return fail(FAOCTASR_EINVAL, "ffl_fwd: null pointer");
    int rc = ffl_check("ffl_fwd", workspace, N, C, H, W, alpha);
    if (rc) return rc;
    const FflWs p = ffl_ws(workspace, N, C, H, W);
    const long imgs = (long)N * C;
    // row pass [P | Q] = X [C_W | S_W]: x and y as the two batch entries of one launch (the stride is their address difference)
    const intptr_t diff = (intptr_t)y - (intptr_t)x;
    if (diff % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "ffl_fwd: x and y are not 4-byte aligned to each other");
    rc = faoctasr_sgemm_batched(x, tabW, p.pq, (int)(imgs * H), 2 * W, W, W, 2 * W, 2 * W, (long)(diff / (intptr_t)sizeof(float)), 0,
                                imgs * H * 2 * W, 2, stream);
    if (rc) return rc;
    const int form = ffl_form(alpha);
    const double hw = (double)H * (double)W;
    dim3 grid((W + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(ffl_col_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p.pq, tabH, planes, p.part, H, W, imgs,
                       (float)(1.0 / sqrt(hw)), form, 0.5f * alpha, log_matrix ? 1 : 0);
    rc = check_launch("ffl_fwd (column pass)");
    if (rc) return rc;
    // 1 / phi(M) per plane follows the planes in the caller's buffer
    hipLaunchKernelGGL(ffl_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)p.part, p.stats,
                       planes ? planes + 2 * imgs * H * W : nullptr, loss, imgs, (long)grid.x * grid.y, (double)imgs * hw, form,
                       0.5 * (double)alpha, log_matrix ? 1 : 0, batch_matrix ? 1 : 0);
    return check_launch("ffl_fwd (finish)");
}

extern "C" int faoctasr_ffl_bwd(const float* g, const float* planes, const float* tabH, const float* tabW, float alpha, int log_matrix,
                                float* dx, float* dy, float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream) {
    if (!g || !planes || !tabH || !tabW || !workspace) return fail(FAOCTASR_EINVAL, "ffl_bwd: null pointer");
    int rc = ffl_check("ffl_bwd", workspace, N, C, H, W, alpha);
    if (rc) return rc;
    if (!dx && !dy) return FAOCTASR_OK;
    const FflWs p = ffl_ws(workspace, N, C, H, W);
    const long imgs = (long)N * C;
    const double hw = (double)H * (double)W;
    // the transform runs once, for the side that is wanted (dx when both are): dL/dy = -dL/dx
    const double coef = (dx ? 2.0 : -2.0) / ((double)imgs * hw * sqrt(hw));
    dim3 grid((W + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(ffl_col_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, planes, planes + 2 * imgs * H * W, tabH, g, p.pq, H, W,
                       (float)coef, ffl_form(alpha), 0.5f * alpha, log_matrix ? 1 : 0);
    rc = check_launch("ffl_bwd (column pass)");
    if (rc) return rc;
    // dX = [T1 | T2] [C_W ; S_W]: the stacked table is the second half of the table buffer
    float* first = dx ? dx : dy;
    rc = faoctasr_sgemm_batched(p.pq, tabW + 2L * W * W, first, (int)(imgs * H), W, 2 * W, 2 * W, W, W, 0, 0, 0, 1, stream);
    if (rc || !(dx && dy)) return rc;
    const long n = imgs * H * W;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(negate_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (const float*)dx,
                       dy, n);
    return check_launch("ffl_bwd (negation)");
}

extern "C" long faoctasr_sprof_workspace_floats(int sides, int N, int C, int H, int W, int Wh, int K) {
    if (sides < 1 || sides > 2) {
        fail(FAOCTASR_EINVAL, "sprof_workspace_floats: sides %d is neither 1 nor 2", sides);
        return -1;
    }
    if (sprof_check("sprof_workspace_floats", sides, N, C, H, W, Wh, K)) return -1;
    return sprof_ws(nullptr, sides, (long)N * C, H, Wh, K).total;
}

extern "C" int faoctasr_sprof_profile_fwd(const float* x, const float* tabH, const float* halfW, const int* csr_off, const int* csr_idx,
                                          const int* cnt, float* A, float* save, float* workspace, int N, int C, int H, int W, int Wh, int K,
                                          faoctasr_stream_t stream) {
    if (!x || !tabH || !halfW || !csr_off || !csr_idx || !cnt || !A || !workspace) return fail(FAOCTASR_EINVAL, "sprof_profile_fwd: null pointer");
    int rc = sprof_check("sprof_profile_fwd", 1, N, C, H, W, Wh, K);
    if (rc) return rc;
    const SprofWs p = sprof_ws(workspace, 1, (long)N * C, H, Wh, K);
    return sprof_profiles("sprof_profile_fwd", x, nullptr, tabH, halfW, csr_off, csr_idx, cnt, A, save, nullptr, p, N, C, H, W, Wh, K,
                          (hipStream_t)stream);
}

extern "C" int faoctasr_sprof_loss_fwd(const float* x, const float* y, const float* tabH, const float* halfW, const int* csr_off,
                                       const int* csr_idx, const int* cnt, double eps, int k_min, int batch_profile, int per_image, float* loss,
                                       float* loss_per_image, float* A, float* save_x, float* save_y, float* workspace, int N, int C, int H,
                                       int W, int Wh, int K, faoctasr_stream_t stream) {
    if (!x || !y || !tabH || !halfW || !csr_off || !csr_idx || !cnt || !loss || !A || !workspace)
        return fail(FAOCTASR_EINVAL, "sprof_loss_fwd: null pointer");
    int rc = sprof_check("sprof_loss_fwd", 2, N, C, H, W, Wh, K);
    if (rc) return rc;
    if (!(eps > 0.0) || eps > 1.0e300) return fail(FAOCTASR_EINVAL, "sprof_loss_fwd: eps %g must be finite and > 0", eps);
    if (k_min < 0 || k_min >= K) return fail(FAOCTASR_EINVAL, "sprof_loss_fwd: k_min %d outside [0, %d)", k_min, K);
    if (per_image && (batch_profile || !loss_per_image))
        return fail(FAOCTASR_EINVAL, "sprof_loss_fwd: per_image needs loss_per_image and excludes batch_profile");
    const long imgs = (long)N * C;
    const SprofWs p = sprof_ws(workspace, 2, imgs, H, Wh, K);
    rc = sprof_profiles("sprof_loss_fwd", x, y, tabH, halfW, csr_off, csr_idx, cnt, A, save_x, save_y, p, N, C, H, W, Wh, K, (hipStream_t)stream);
    if (rc) return rc;
    // the coefficient table of a side follows its saved planes
    const long planes = imgs * 2 * H * Wh;
    hipLaunchKernelGGL(sprof_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)A, cnt, loss, loss_per_image,
                       save_x ? save_x + planes : nullptr, save_y ? save_y + planes : nullptr, N, C, K, k_min, eps, batch_profile ? 1 : 0,
                       per_image ? 1 : 0);
    return check_launch("sprof_loss_fwd (finish)");
}

extern "C" int faoctasr_sprof_bwd(const float* g, int g_per_image, const float* gA, const float* save_x, const float* save_y, const float* tabH,
                                  const float* halfW, const short* binmap, const int* cnt, float* dx, float* dy, float* workspace, int N, int C,
                                  int H, int W, int Wh, int K, faoctasr_stream_t stream) {
    if (!tabH || !halfW || !binmap || !cnt || !workspace) return fail(FAOCTASR_EINVAL, "sprof_bwd: null pointer");
    if (!g == !gA) return fail(FAOCTASR_EINVAL, "sprof_bwd: exactly one of g (the loss) and gA (the profile) must be given");
    int rc = sprof_check("sprof_bwd", gA ? 1 : 2, N, C, H, W, Wh, K);
    if (rc) return rc;
    if (gA && dy) return fail(FAOCTASR_EINVAL, "sprof_bwd: the profile has one input");
    if ((dx && !save_x) || (dy && !save_y)) return fail(FAOCTASR_EINVAL, "sprof_bwd: a gradient is wanted for a side the forward saved nothing for");
    if (!dx && !dy) return FAOCTASR_OK;
    const long imgs = (long)N * C, planes = imgs * 2 * H * Wh;
    const hipStream_t st = (hipStream_t)stream;
    const SprofWs p = sprof_ws(workspace, gA ? 1 : 2, imgs, H, Wh, K);
    const float* coef_x = dx ? save_x + planes : nullptr;
    const float* coef_y = dy ? save_y + planes : nullptr;
    if (gA) {
        const long n = imgs * K;
        hipLaunchKernelGGL(sprof_cotangent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gA, cnt, p.coef, n, K);
        rc = check_launch("sprof_bwd (cotangent)");
        if (rc) return rc;
        coef_x = p.coef;
    }
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(sprof_col_bwd_kernel, grid, dim3(256), 0, st, save_x, save_y, coef_x, coef_y, binmap, tabH, g, g_per_image ? 1 : 0, p.pq,
                       H, W, Wh, C, K, imgs, (float)(2.0 / ((double)H * (double)W)), dx ? 1 : 0, dy ? 1 : 0);
    rc = check_launch("sprof_bwd (column pass)");
    if (rc) return rc;
    // dX = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]: the transposed half table follows the forward one
    const float* stacked = halfW + 2L * W * Wh;
    const long sT = imgs * H * 2 * Wh;
    if (dx && dy) {
        const intptr_t diff = (intptr_t)dy - (intptr_t)dx;
        if (diff % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "sprof_bwd: dx and dy are not 4-byte aligned to each other");
        return faoctasr_sgemm_batched(p.pq, stacked, dx, (int)(imgs * H), W, 2 * Wh, 2 * Wh, W, W, sT, 0, (long)(diff / (intptr_t)sizeof(float)), 2,
                                      stream);
    }
    return faoctasr_sgemm_batched(dx ? p.pq : p.pq + sT, stacked, dx ? dx : dy, (int)(imgs * H), W, 2 * Wh, 2 * Wh, W, W, 0, 0, 0, 1, stream);
}

extern "C" long faoctasr_frc_workspace_floats(int N, int C, int H, int W, int Wh, int K) {
    if (sprof_check("frc_workspace_floats", 2, N, C, H, W, Wh, K)) return -1;
    return frc_ws(nullptr, (long)N * C, H, Wh).total;
}

extern "C" int faoctasr_frc_fwd(const float* x, const float* y, const float* tabH, const float* halfW, const int* csr_off, const int* csr_idx,
                                const int* cnt, double eps, int k_min, int k_max, int per_image, float* index, float* index_per_image,
                                float* curve, float* rings, float* save, float* workspace, int N, int C, int H, int W, int Wh, int K,
                                faoctasr_stream_t stream) {
    if (!x || !y || !tabH || !halfW || !csr_off || !csr_idx || !cnt || !index || !curve || !rings || !workspace)
        return fail(FAOCTASR_EINVAL, "frc_fwd: null pointer");
    int rc = sprof_check("frc_fwd", 2, N, C, H, W, Wh, K);
    if (rc) return rc;
    if (!(eps > 0.0) || eps > 1.0e300) return fail(FAOCTASR_EINVAL, "frc_fwd: eps %g must be finite and > 0", eps);
    if (k_min < 0 || k_max < k_min || k_max > K - 1)
        return fail(FAOCTASR_EINVAL, "frc_fwd: the band k_min %d, k_max %d must satisfy 0 <= k_min <= k_max <= %d", k_min, k_max, K - 1);
    if (per_image && !index_per_image) return fail(FAOCTASR_EINVAL, "frc_fwd: per_image needs index_per_image");
    const long imgs = (long)N * C;
    const hipStream_t st = (hipStream_t)stream;
    const FrcWs p = frc_ws(workspace, imgs, H, Wh);
    const intptr_t d = (intptr_t)y - (intptr_t)x;
    if (d % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "frc_fwd: x and y are not 4-byte aligned to each other");
    rc = faoctasr_sgemm_batched(x, halfW, p.pq, (int)(imgs * H), 2 * Wh, W, W, 2 * Wh, 2 * Wh, (long)(d / (intptr_t)sizeof(float)), 0,
                                imgs * H * 2 * Wh, 2, stream);
    if (rc) return rc;
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(frc_col_fwd_kernel, grid, dim3(256), 0, st, (const float*)p.pq, tabH, p.pw, save, H, W, Wh, imgs);
    rc = check_launch("frc_fwd (column pass)");
    if (rc) return rc;
    const long waves = 3 * imgs * K;
    hipLaunchKernelGGL(sprof_bin_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, (const float*)p.pw, csr_off, csr_idx, cnt, rings,
                       3 * imgs, K, (long)H * Wh);
    rc = check_launch("frc_fwd (ring sums)");
    if (rc) return rc;
    // the coefficient tables follow the saved planes
    hipLaunchKernelGGL(frc_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)rings, cnt, index, index_per_image, curve,
                       save ? save + imgs * 4 * H * Wh : nullptr, N, C, K, k_min, k_max, eps, per_image ? 1 : 0);
    return check_launch("frc_fwd (finish)");
}

extern "C" int faoctasr_frc_bwd(const float* g, int g_per_image, const float* save, const float* tabH, const float* halfW, const short* binmap,
                                float* dx, float* dy, float* workspace, int N, int C, int H, int W, int Wh, int K, faoctasr_stream_t stream) {
    if (!g || !tabH || !halfW || !binmap || !workspace) return fail(FAOCTASR_EINVAL, "frc_bwd: null pointer");
    int rc = sprof_check("frc_bwd", 2, N, C, H, W, Wh, K);
    if (rc) return rc;
    if ((dx || dy) && !save) return fail(FAOCTASR_EINVAL, "frc_bwd: a gradient is wanted but the forward saved nothing");
    if (!dx && !dy) return FAOCTASR_OK;
    const long imgs = (long)N * C;
    const FrcWs p = frc_ws(workspace, imgs, H, Wh);
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(frc_col_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, save, save + imgs * 4 * H * Wh, binmap, tabH, g,
                       g_per_image ? 1 : 0, p.pq, H, W, Wh, C, K, imgs, (float)(1.0 / ((double)H * (double)W)), dx ? 1 : 0, dy ? 1 : 0);
    rc = check_launch("frc_bwd (column pass)");
    if (rc) return rc;
    // dX = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]: the transposed half table follows the forward one
    const float* stacked = halfW + 2L * W * Wh;
    const long sT = imgs * H * 2 * Wh;
    if (dx && dy) {
        const intptr_t diff = (intptr_t)dy - (intptr_t)dx;
        if (diff % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "frc_bwd: dx and dy are not 4-byte aligned to each other");
        return faoctasr_sgemm_batched(p.pq, stacked, dx, (int)(imgs * H), W, 2 * Wh, 2 * Wh, W, W, sT, 0, (long)(diff / (intptr_t)sizeof(float)), 2,
                                      stream);
    }
    return faoctasr_sgemm_batched(dx ? p.pq : p.pq + sT, stacked, dx ? dx : dy, (int)(imgs * H), W, 2 * Wh, 2 * Wh, W, W, 0, 0, 0, 1, stream);
}

static int pcorr_check(const char* what, int N, int C, int H, int W, int Wh, int K, int U) {
    int rc = sprof_check(what, 2, N, C, H, W, Wh, K);
    if (rc) return rc;
    if (Wh != W / 2 + 1) return fail(FAOCTASR_EINVAL, "%s: Wh %d is not W/2 + 1 = %d", what, Wh, W / 2 + 1);
    if (U < 1 || U > 100) return fail(FAOCTASR_EINVAL, "%s: upsample %d outside 1..100", what, U);
    return FAOCTASR_OK;
}

// launches 5 to 8 of phase correlation: the coarse peak of the (unscaled) surface, the twiddles, the two contractions
static int pcorr_peak(const PcorrWs& p, const float* surf, float* shift, float* peak, int N, int C, int H, int W, int Wh, int upsample,
                      int max_shift_y, int max_shift_x, const float* tabH, hipStream_t st) {
    int rc;
    hipLaunchKernelGGL(pcorr_peak_kernel, dim3((unsigned)N), dim3(256), 0, st, (const float*)surf, p.coarse, shift, peak, H, W, C, max_shift_y,
                       max_shift_x);
    rc = check_launch("pcorr_fwd (peak)");
    if (rc || upsample == 1) return rc;
    const int T = pcorr_points(upsample);
    const long tw = (long)(H + Wh) * T;
    hipLaunchKernelGGL(pcorr_twiddle_kernel, dim3((unsigned)((tw + 255) / 256), (unsigned)N), dim3(256), 0, st, (const int*)p.coarse, p.ey, p.ex, H,
                       W, Wh, upsample, T);
    rc = check_launch("pcorr_fwd (twiddles)");
    if (rc) return rc;
    dim3 gridT((Wh + PH_T - 1) / PH_T, (T + PH_T - 1) / PH_T, (unsigned)N);
    hipLaunchKernelGGL(hspec_inv_col_kernel, gridT, dim3(256), 0, st, (const float*)p.rn, (const float*)p.ey, (long)H * 2 * T, T, 2 * T,
                       (const float*)nullptr, 0.f, 1.f, p.up, H, W, Wh, C, 1);
    rc = check_launch("pcorr_fwd (T x H x Wh contraction)");
    if (rc) return rc;
    hipLaunchKernelGGL(pcorr_refine_kernel, dim3((unsigned)N), dim3(256), 0, st, (const float*)p.up, (const float*)p.ex, (const int*)p.coarse,
                       shift, peak, Wh, (double)H * (double)W * (double)C, upsample, T);
    return check_launch("pcorr_fwd (T x Wh x T contraction)");
}

extern "C" long faoctasr_pcorr_workspace_floats(int N, int C, int H, int W, int Wh, int K, int upsample) {
    if (pcorr_check("pcorr_workspace_floats", N, C, H, W, Wh, K, upsample)) return -1;
    return pcorr_ws(nullptr, N, C, H, W, Wh, upsample).total;
}

extern "C" int faoctasr_pcorr_fwd(const float* a, const float* b, const float* tabH, const float* halfW, const short* binmap, double eps,
                                  int k_max, int normalize, int upsample, int max_shift_y, int max_shift_x, float* shift, float* peak,
                                  float* surface, float* workspace, int N, int C, int H, int W, int Wh, int K, faoctasr_stream_t stream) {
    if (!a || !b || !tabH || !halfW || !binmap || !workspace) return fail(FAOCTASR_EINVAL, "pcorr_fwd: null pointer");
    if (!shift != !peak || (!shift && !surface)) return fail(FAOCTASR_EINVAL, "pcorr_fwd: shift and peak go together, and without them the surface is the output");
    int rc = pcorr_check("pcorr_fwd", N, C, H, W, Wh, K, upsample);
    if (rc) return rc;
    if (!(eps >= 0.0) || eps > 1.0e30) return fail(FAOCTASR_EINVAL, "pcorr_fwd: eps %g must be finite and >= 0", eps);
    if (k_max < 0 || k_max > K - 1) return fail(FAOCTASR_EINVAL, "pcorr_fwd: k_max %d outside 0..%d", k_max, K - 1);
    if (max_shift_y < 0 || max_shift_y > H / 2 || max_shift_x < 0 || max_shift_x > W / 2)
        return fail(FAOCTASR_EINVAL, "pcorr_fwd: max_shift (%d, %d) outside 0..%d, 0..%d", max_shift_y, max_shift_x, H / 2, W / 2);
    const long imgs = (long)N * C;
    const hipStream_t st = (hipStream_t)stream;
    const PcorrWs p = pcorr_ws(workspace, N, C, H, W, Wh, upsample);
    const intptr_t d = (intptr_t)b - (intptr_t)a;
    if (d % (intptr_t)sizeof(float)) return fail(FAOCTASR_EINVAL, "pcorr_fwd: a and b are not 4-byte aligned to each other");
    rc = faoctasr_sgemm_batched(a, halfW, p.pq, (int)(imgs * H), 2 * Wh, W, W, 2 * Wh, 2 * Wh, (long)(d / (intptr_t)sizeof(float)), 0,
                                imgs * H * 2 * Wh, 2, stream);
    if (rc) return rc;
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(pcorr_col_fwd_kernel, grid, dim3(256), 0, st, (const float*)p.pq, tabH, binmap, p.rn, H, W, Wh, imgs, (float)eps, k_max,
                       normalize ? 1 : 0);
    rc = check_launch("pcorr_fwd (column pass)");
    if (rc) return rc;
    // the inverse on the channel sum: [T1 | T2] over [P | Q], then X = [T1 | T2] [C_W[:, :Wh]^T ; S_W[:, :Wh]^T]
    grid.z = (unsigned)N;
    hipLaunchKernelGGL(hspec_inv_col_kernel, grid, dim3(256), 0, st, (const float*)p.rn, tabH, 0L, H, 2 * H, (const float*)nullptr, 0.f, 1.f, p.pq, H,
                       W, Wh, C, 1);
    rc = check_launch("pcorr_fwd (inverse column pass)");
    if (rc) return rc;
    float* surf = surface ? surface : p.surf;
    rc = faoctasr_sgemm_batched(p.pq, halfW + 2L * W * Wh, surf, N * H, W, 2 * Wh, 2 * Wh, W, W, 0, 0, 0, 1, stream);
    if (rc) return rc;
    if (shift) rc = pcorr_peak(p, surf, shift, peak, N, C, H, W, Wh, upsample, max_shift_y, max_shift_x, tabH, st);
    if (rc || !surface) return rc;
    const long ns = (long)N * H * W;
    hipLaunchKernelGGL(pcorr_scale_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, surface, ns, (float)(H * W));
    return check_launch("pcorr_fwd (surface scale)");
}

// the Fourier shift has no rings, but shares sprof_check: the ring count of a legal shape, 0 (refused on the shape) otherwise
static int fshift_bins(int H, int W) { return (H >= 2 && W >= 2 && H <= 1024 && W <= 1024) ? sprof_bins(H, W) : 0; }

extern "C" long faoctasr_fourier_shift_workspace_floats(int N, int C, int H, int W) {
    if (sprof_check("fourier_shift_workspace_floats", 1, N, C, H, W, W / 2 + 1, fshift_bins(H, W))) return -1;
    return fshift_ws(nullptr, (long)N * C, H, W / 2 + 1).total;
}

extern "C" int faoctasr_fourier_shift(const float* x, const float* shift, float sign, const float* tabH, const float* halfW, float* out,
                                      float* workspace, int N, int C, int H, int W, faoctasr_stream_t stream) {
    if (!x || !shift || !tabH || !halfW || !out || !workspace) return fail(FAOCTASR_EINVAL, "fourier_shift: null pointer");
    const int Wh = W / 2 + 1;
    int rc = sprof_check("fourier_shift", 1, N, C, H, W, Wh, fshift_bins(H, W));
    if (rc) return rc;
    if (sign != 1.f && sign != -1.f) return fail(FAOCTASR_EINVAL, "fourier_shift: sign %g is neither 1 nor -1", (double)sign);
    const long imgs = (long)N * C;
    const hipStream_t st = (hipStream_t)stream;
    const FshiftWs p = fshift_ws(workspace, imgs, H, Wh);
    rc = faoctasr_sgemm_batched(x, halfW, p.pq, (int)(imgs * H), 2 * Wh, W, W, 2 * Wh, 2 * Wh, 0, 0, 0, 1, stream);
    if (rc) return rc;
    dim3 grid((Wh + PH_T - 1) / PH_T, (H + PH_T - 1) / PH_T, (unsigned)imgs);
    hipLaunchKernelGGL(sprof_col_fwd_kernel<1>, grid, dim3(256), 0, st, (const float*)p.pq, tabH, p.pw, p.planes, (float*)nullptr, H, W, Wh, imgs);
    rc = check_launch("fourier_shift (column pass)");
    if (rc) return rc;
    hipLaunchKernelGGL(hspec_inv_col_kernel, grid, dim3(256), 0, st, (const float*)p.planes, tabH, 0L, H, 2 * H, shift, sign,
                       (float)(1.0 / ((double)H * (double)W)), p.pq, H, W, Wh, C, 0);
    rc = check_launch("fourier_shift (inverse column pass)");
    if (rc) return rc;
    return faoctasr_sgemm_batched(p.pq, halfW + 2L * W * Wh, out, (int)(imgs * H), W, 2 * Wh, 2 * Wh, W, W, 0, 0, 0, 1, stream);
}
