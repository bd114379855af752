// Differentiable mutual information of two images (Gaussian Parzen windows, soft joint histogram) on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32).  Not part of the reference, whose NMI (utils.py:209-212, csrc/eval.hip) is a hard histogram.
//
// Per (n, c) plane with n_pix pixels, K bins of width d over [lo, hi], centres c_k = lo + (k + 1/2) d, sigma = r d:
//   Wa[p, k] = softmax_k(-(x_p - c_k)^2 / (2 sigma^2)),  Wb likewise from y,  P = Wa^T Wb / n_pix  (K x K),
//   pa = row sums, pb = column sums, H(q) = -sum q log(q + eps),  MI = Ha + Hb - Hab,  NMI = (Ha + Hb) / Hab.
// Nothing of size pixels x bins is ever stored: the weights live in registers / LDS and are recomputed in the backward.
//
// The weights.  In bin coordinates t = (x - lo) / d - 1/2 the logit of bin k is -(t - k)^2 / (2 r^2).  k* = the nearest bin
// (clamped to [0, K-1]) has the largest logit.  With delta = (x - c_k*) / d -- the subtraction of the nearby centre is exact, so
// delta keeps the input's own precision, which t (x + 1 rounds) does not -- and n = k - k*, logit_k - logit_k* =
// n (2 delta - n) / (2 r^2) <= 0 is formed from small numbers: the softmax is stable and accurate for any finite x, inside the
// range or far outside it.
//
// mi_hist.  A block takes MI_CHUNK = 2048 pixels of one plane, each of its four waves one chain of MI_CHAIN = 512.  A wave
// stages the normalised weights of 16 pixels of both images in LDS (a lane forms half the bins of one pixel of one image; the
// two halves exchange their sums by one cross-lane move), then feeds them to the MFMA as A = Wa^T (bins x pixels) and
// B = Wb (pixels x bins): one 32 x 32 accumulator tile for K <= 32, four for K <= 64.  Bins beyond K and pixels beyond the plane
// carry weight exactly 0.  The four chains are added as (w0 + w1) + (w2 + w3) and the block writes one K x K partial: no
// atomics, and both constants belong to the kernel, so the result does not depend on the grid.
// mi_final.  Per plane: the partials added in chunk order in double, marginals, entropies, score, and (when a backward can
// follow) the table G = dS/dP with 1 / (D n_pix sigma^2) folded in.  Every sum is invariant under transposing P -- (i, j) is
// paired with (j, i), Ha + Hb and u_i + v_j are commutative pairs -- so S(x, y) == S(y, x) and G(y, x) == G(x, y)^T bit for bit.
// mi_grad.  dS/dx_p = g / (D n_pix sigma^2) sum_k Wa[p,k] (c_k - xbar_p) sum_j G_kj Wb[p,j].  The inner product is a
// (K x K) x (K x 32 pixels) GEMM on the MFMA: a lane holds the weights of pixel (lane & 31) for exactly the bins whose rows of
// the 32 x 32 result land in its accumulator registers, so the B operand comes straight from registers, the result meets the
// other image's weights register by register, and only G lives in LDS.  One device function forms both sides (dy: G read
// transposed).  The file is compiled without contraction so that the two instantiations round alike.
#include "common.h"

#pragma clang fp contract(off)

using namespace faoctasr;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MI_CHUNK = 2048;      // pixels per block of mi_hist (a constant of the kernel: the partials' layout depends on it)
constexpr int MI_CHAIN = 512;       // pixels per wave: the longest fp32 accumulation chain
constexpr int MI_SUB = 16;          // pixels a wave stages at a time
constexpr int MI_GCHUNK = 1024;     // pixels per block of mi_grad
constexpr int MI_MAX_BINS = 64;

struct MiBins {
    float lo, d, invd, a2;          // range start, bin width, 1 / bin width, log2(e) / (2 sigma_ratio^2)
    int K;
};

// the bin of a lane's i-th weight.  LAYOUT 0: lane half h holds bins [h NB, (h + 1) NB).  LAYOUT 1: the rows of the MFMA's
// 32 x 32 result that lane half h holds (row = (r & 3) + 8 (r >> 2) + 4 h in register r), one tile of 32 bins after the other
template <int LAYOUT>
__device__ __forceinline__ int mi_bin(int i, int h, int NB) {
    return LAYOUT == 0 ? h * NB + i : 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * h;
}

// NB of the KP = 2 NB weights of one pixel (the lanes l and l ^ 32 hold the two halves); kstar: the nearest bin; invalid pixels
// and bins >= K get exactly 0
template <int NB, int LAYOUT>
__device__ __forceinline__ void mi_weights(float x, bool valid, const MiBins& b, int h, float (&w)[NB], float& kstar) {
    kstar = fminf(fmaxf(rintf((x - b.lo) * b.invd - 0.5f), 0.f), (float)(b.K - 1));
    // clamped to the finite range: for |x| near FLT_MAX / invd the product overflows, and bin k* would get 0 * inf
    const float delta2 = fminf(fmaxf(2.f * ((x - fmaf(kstar + 0.5f, b.d, b.lo)) * b.invd), -3.0e38f), 3.0e38f);
    // K behind an empty asm: otherwise the per-lane masks of `k < K` are hoisted out of the pixel loop, one SGPR pair per bin,
    // and spill
    int K = b.K;
    asm volatile("" : "+s"(K));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int k = mi_bin<LAYOUT>(i, h, NB);
        const float fk = (float)k;
        const float n = fk - kstar;
        const float e = (valid && k < K) ? exp2f(b.a2 * (n * (delta2 - n))) : 0.f;
        w[i] = e;
        s += e;
    }
    s = s + __shfl_xor(s, 32, 64);          // commutative: both halves hold the same sum
    const float inv = valid ? 1.f / s : 0.f;    // s >= 1: bin k* contributes exp2(0)
#pragma unroll
    for (int i = 0; i < NB; ++i) w[i] *= inv;
}

template <int KP>
__global__ __launch_bounds__(256) void mi_hist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      float* __restrict__ part, long n_pix, const MiBins b) {
    constexpr int NB = KP / 2, T = KP / 32, RS = 2 * MI_SUB + 1;    // row of a bin: 16 pixels of x, 16 of y, one pad
    __shared__ float Ws[4 * KP * RS];                               // >= 2 KP KP floats: reused to add the four chains
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pix = lane & 15, img = (lane >> 4) & 1, h = lane >> 5, l31 = lane & 31;
    const long plane = blockIdx.y, chunk0 = (long)blockIdx.x * MI_CHUNK;
    const long left = n_pix - chunk0;
    const int cnt = left < MI_CHUNK ? (int)left : MI_CHUNK;
    const int iters = ((cnt < MI_CHAIN ? cnt : MI_CHAIN) + MI_SUB - 1) / MI_SUB;    // the same for the four waves (wave 0 has the most)
    const int wcnt = cnt - wave * MI_CHAIN;                         // this wave's valid pixels (may be <= 0)
    const float* src = (img ? y : x) + plane * n_pix + chunk0 + wave * MI_CHAIN;
    float* W = Ws + wave * KP * RS;
    f32x16 acc[T * T];
#pragma unroll
    for (int t = 0; t < T * T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float next = pix < wcnt ? src[pix] : 0.f;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int p = it * MI_SUB + pix;
        const float cur = next;
        next = (it + 1 < iters && p + MI_SUB < wcnt) ? src[p + MI_SUB] : 0.f;     // in flight while this sub-tile is worked on
        float w[NB], kstar;
        mi_weights<NB, 0>(cur, p < wcnt, b, h, w, kstar);
        __syncthreads();                                            // the previous sub-tile has been read
#pragma unroll
        for (int i = 0; i < NB; ++i) W[(h * NB + i) * RS + l31] = w[i];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MI_SUB; kk += 2) {
            float a[T], bb[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                a[t] = W[(32 * t + l31) * RS + kk + h];
                bb[t] = W[(32 * t + l31) * RS + MI_SUB + kk + h];
            }
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = 0; tj < T; ++tj)
                    acc[ti * T + tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti], bb[tj], acc[ti * T + tj], 0, 0, 0);
        }
    }
    // (w0 + w1) + (w2 + w3): waves 0 and 2 store, waves 1 and 3 add, then every thread adds the two halves
    float* buf = Ws + (wave >> 1) * KP * KP;
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if ((wave & 1) == pass) {
#pragma unroll
            for (int t = 0; t < T * T; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = 32 * (t / T) + (r & 3) + 8 * (r >> 2) + 4 * h, j = 32 * (t % T) + l31;
                    buf[i * KP + j] = pass ? buf[i * KP + j] + acc[t][r] : acc[t][r];
                }
        }
        __syncthreads();
    }
    const int K = b.K;
    float* out = part + (plane * gridDim.x + blockIdx.x) * (long)(K * K);
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, j = e - i * K;
        out[e] = Ws[i * KP + j] + Ws[KP * KP + i * KP + j];
    }
}

// -q log(q + eps)'s negative and the derivative's negative: h(q) = q log(q + eps), a(q) = log(q + eps) + q / (q + eps)
__device__ __forceinline__ double mi_h(double q, double eps) { return q * log(q + eps); }
__device__ __forceinline__ double mi_a(double q, double eps) { return log(q + eps) + q / (q + eps); }

// one block per plane.  score[plane] in double; table (may be nullptr): G scaled by `fold`
__global__ __launch_bounds__(256) void mi_final_kernel(const float* __restrict__ part, double* __restrict__ score,
                                                       float* __restrict__ table, int K, long chunks, double n_pix, double eps,
                                                       int normalized, double fold) {
    __shared__ double P[MI_MAX_BINS * MI_MAX_BINS];
    __shared__ double pa[MI_MAX_BINS], pb[MI_MAX_BINS], ua[MI_MAX_BINS], vb[MI_MAX_BINS], ha[MI_MAX_BINS], hb[MI_MAX_BINS];
    __shared__ double red[256], ent[2];
    const int tid = threadIdx.x, KK = K * K;
    const long plane = blockIdx.x;
    const float* src = part + plane * chunks * KK;
    for (int e = tid; e < KK; e += 256) {
        double s = 0.0;
        for (long c = 0; c < chunks; ++c) s += (double)src[c * KK + e];
        P[e] = s / n_pix;
    }
    __syncthreads();
    if (tid < 2 * K) {                     // thread i: row sum i; thread K + j: column sum j; both in index order
        const int i = tid < K ? tid : tid - K;
        const int st = tid < K ? 1 : K, o = tid < K ? i * K : i;
        double s = 0.0;
        for (int j = 0; j < K; ++j) s += P[o + j * st];
        (tid < K ? pa : pb)[i] = s;
        (tid < K ? ua : vb)[i] = -mi_a(s, eps);
        (tid < K ? ha : hb)[i] = mi_h(s, eps);
    }
    // sum over the unordered pairs {i, j}: the diagonal alone, (i, j) + (j, i) otherwise
    double acc = 0.0;
    for (int e = tid; e < KK; e += 256) {
        const int i = e / K, j = e - i * K;
        if (i == j) acc += mi_h(P[e], eps);
        else if (i < j) acc += mi_h(P[e], eps) + mi_h(P[j * K + i], eps);
    }
    const double Hab = -block_tree_256(acc, red);
    if (tid < 2) {
        const double* hh = tid ? hb : ha;
        double s = 0.0;
        for (int i = 0; i < K; ++i) s += hh[i];
        ent[tid] = -s;
    }
    __syncthreads();
    const double Hm = ent[0] + ent[1];
    if (tid == 0) score[plane] = normalized ? Hm / Hab : Hm - Hab;
    if (table) {
        const double cu = normalized ? 1.0 / Hab : 1.0, ca = normalized ? Hm / (Hab * Hab) : 1.0;
        float* G = table + plane * KK;
        for (int e = tid; e < KK; e += 256) {
            const int i = e / K, j = e - i * K;
            G[e] = (float)(fold * (ca * mi_a(P[e], eps) + cu * (ua[i] + vb[j])));
        }
    }
}

// single block: out[n] = mean over c (per_image) or out[0] = mean over all planes, in plane order in double
__global__ __launch_bounds__(256) void mi_mean_kernel(const double* __restrict__ score, float* __restrict__ out, long N, long C,
                                                      int per_image) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if (per_image) {
        for (long n = tid; n < N; n += 256) {
            double s = 0.0;
            for (long c = 0; c < C; ++c) s += score[n * C + c];
            out[n] = (float)(s / (double)C);
        }
        return;
    }
    const double s = block_tree_256(strided_sum_256(score, N * C), red);
    if (tid == 0) out[0] = (float)(s / (double)(N * C));
}

// one side's derivative for the pixel (lane & 31): sum_k ws_k ((k - k*) - m) sum_j G_kj wo_j, m = sum_k ws_k (k - k*), with
// G_kj read as Gs[k][j] (TR false: dx) or Gs[j][k] (TR true: dy).  ws: this side's weights, wo: the other image's.
template <int KP, bool TR>
__device__ __forceinline__ float mi_side(const float* Gs, const float (&ws)[KP / 2], const float (&wo)[KP / 2], float kstar, int h,
                                         int l31) {
    constexpr int NB = KP / 2, T = KP / 32, GS = KP + 1;
    f32x16 r[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) r[t][q] = 0.f;
#pragma unroll
    for (int s = 0; s < NB; ++s) {                      // reduction step: lane half h brings bin mi_bin<1>(s, h) of the other image
        const int jb = mi_bin<1>(s, h, NB);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float a = TR ? Gs[jb * GS + 32 * t + l31] : Gs[(32 * t + l31) * GS + jb];
            r[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wo[s], r[t], 0, 0, 0);
        }
    }
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) m += ws[i] * ((float)mi_bin<1>(i, h, NB) - kstar);
    m = m + __shfl_xor(m, 32, 64);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) acc += (ws[i] * (((float)mi_bin<1>(i, h, NB) - kstar) - m)) * r[i >> 4][i & 15];
    return acc + __shfl_xor(acc, 32, 64);
}

template <int KP>
__global__ __launch_bounds__(256) void mi_grad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ table, const float* __restrict__ g,
                                                      float* __restrict__ dx, float* __restrict__ dy, long n_pix, long C,
                                                      int per_image, const MiBins b) {
    constexpr int NB = KP / 2, GS = KP + 1;
    __shared__ float Gs[KP * GS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const long plane = blockIdx.y;
    const int K = b.K;
    const float* G = table + plane * (long)(K * K);
    for (int e = tid; e < KP * KP; e += 256) {
        const int i = e / KP, j = e - i * KP;
        Gs[i * GS + j] = (i < K && j < K) ? G[i * K + j] : 0.f;
    }
    __syncthreads();
    const float gv = g[per_image ? plane / C : 0];
    const long base = (long)blockIdx.x * MI_GCHUNK + wave * (MI_GCHUNK / 4);
#pragma unroll 1
    for (int it = 0; it < MI_GCHUNK / 4 / 32; ++it) {
        const long p0 = base + it * 32;
        if (p0 >= n_pix) break;                         // the same for the whole wave
        const long p = p0 + l31;
        const bool valid = p < n_pix;
        const long o = plane * n_pix + p;
        float wa[NB], wb[NB], ka, kb;
        mi_weights<NB, 1>(valid ? x[o] : 0.f, valid, b, h, wa, ka);
        mi_weights<NB, 1>(valid ? y[o] : 0.f, valid, b, h, wb, kb);
        if (dx) {
            const float v = mi_side<KP, false>(Gs, wa, wb, ka, h, l31);
            if (valid && h == 0) dx[o] = v * gv;
        }
        if (dy) {
            const float v = mi_side<KP, true>(Gs, wb, wa, kb, h, l31);
            if (valid && h == 0) dy[o] = v * gv;
        }
    }
}

struct MiWs {
    double* score;
    float* part;
    long chunks, total;
};

MiWs mi_ws(float* ws, long planes, long n_pix, int K) {
    MiWs p;
    p.chunks = (n_pix + MI_CHUNK - 1) / MI_CHUNK;
    p.score = (double*)ws;
    p.part = ws + 2 * planes;
    p.total = 2 * planes + planes * p.chunks * K * K;
    return p;
}

int mi_check(const char* what, int N, int C, int H, int W, int bins, float lo, float hi, float sigma_ratio) {
    if (N < 1 || C < 1 || H < 1 || W < 1 || (long)H * W > 0x7fffffffL || (long)N * C > 65535)
        return fail(FAOCTASR_EINVAL, "%s: bad shape N %d C %d H %d W %d (N*C <= 65535)", what, N, C, H, W);
    if (bins < 2 || bins > MI_MAX_BINS) return fail(FAOCTASR_EINVAL, "%s: bins must be in [2, %d], got %d", what, MI_MAX_BINS, bins);
    if (!(hi > lo) || !(hi - lo < 3.0e38f)) return fail(FAOCTASR_EINVAL, "%s: value range (%g, %g) is empty or not finite", what, lo, hi);
    if (!(sigma_ratio > 0.f) || !(sigma_ratio < 3.0e38f)) return fail(FAOCTASR_EINVAL, "%s: sigma_ratio must be finite and > 0, got %g", what, sigma_ratio);
    return FAOCTASR_OK;
}

MiBins mi_bins(int bins, float lo, float hi, float sigma_ratio) {
    MiBins b;
    b.lo = lo;
    b.d = (float)(((double)hi - (double)lo) / (double)bins);
    b.invd = (float)((double)bins / ((double)hi - (double)lo));
    b.a2 = (float)(1.4426950408889634 / (2.0 * (double)sigma_ratio * (double)sigma_ratio));
    b.K = bins;
    return b;
}

}  // namespace

extern "C" long faoctasr_mi_workspace_floats(int N, int C, int H, int W, int bins) {
    if (mi_check("mi_workspace_floats", N, C, H, W, bins, 0.f, 1.f, 1.f)) return -1;
    return mi_ws(nullptr, (long)N * C, (long)H * W, bins).total;
}

extern "C" int faoctasr_mi_fwd(const float* x, const float* y, float* out, float* table, float* workspace, int N, int C, int H, int W,
                               int bins, float lo, float hi, float sigma_ratio, float eps, int normalized, int per_image,
                               faoctasr_stream_t stream) {
    if (!x || !y || !out || !workspace) return fail(FAOCTASR_EINVAL, "mi_fwd: null pointer");
    if ((uintptr_t)workspace % 8) return fail(FAOCTASR_EINVAL, "mi_fwd: workspace must be 8-byte aligned");
    int rc = mi_check("mi_fwd", N, C, H, W, bins, lo, hi, sigma_ratio);
    if (rc) return rc;
    if (!(eps > 0.f) || !(eps < 3.0e38f)) return fail(FAOCTASR_EINVAL, "mi_fwd: eps must be finite and > 0, got %g", eps);
    const long planes = (long)N * C, n_pix = (long)H * W;
    const MiWs p = mi_ws(workspace, planes, n_pix, bins);
    const MiBins b = mi_bins(bins, lo, hi, sigma_ratio);
    dim3 grid((unsigned)p.chunks, (unsigned)planes);
    if (bins <= 32) hipLaunchKernelGGL(mi_hist_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, x, y, p.part, n_pix, b);
    else hipLaunchKernelGGL(mi_hist_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, x, y, p.part, n_pix, b);
    rc = check_launch("mi_fwd (histogram)");
    if (rc) return rc;
    // dS/dx carries 1 / (D n_pix sigma^2) and (c_k - xbar) = d (k - kbar): d / (D n_pix r^2 d^2) = invd / (D n_pix r^2), D the
    // number of planes in one mean (all of them, or with per_image the C of one sample)
    const double fold = (double)b.invd / ((double)(per_image ? C : planes) * (double)n_pix * (double)sigma_ratio * (double)sigma_ratio);
    hipLaunchKernelGGL(mi_final_kernel, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, (const float*)p.part, p.score, table,
                       bins, p.chunks, (double)n_pix, (double)eps, normalized ? 1 : 0, fold);
    rc = check_launch("mi_fwd (entropies)");
    if (rc) return rc;
    hipLaunchKernelGGL(mi_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)p.score, out, (long)N, (long)C,
                       per_image ? 1 : 0);
    return check_launch("mi_fwd (mean)");
}

extern "C" int faoctasr_mi_bwd(const float* g, const float* x, const float* y, const float* table, float* dx, float* dy, int N, int C,
                               int H, int W, int bins, float lo, float hi, float sigma_ratio, int per_image,
                               faoctasr_stream_t stream) {
    if (!g || !x || !y || !table) return fail(FAOCTASR_EINVAL, "mi_bwd: null pointer");
    int rc = mi_check("mi_bwd", N, C, H, W, bins, lo, hi, sigma_ratio);
    if (rc) return rc;
    if (!dx && !dy) return FAOCTASR_OK;
    const long planes = (long)N * C, n_pix = (long)H * W;
    const MiBins b = mi_bins(bins, lo, hi, sigma_ratio);
    dim3 grid((unsigned)((n_pix + MI_GCHUNK - 1) / MI_GCHUNK), (unsigned)planes);
    if (bins <= 32)
        hipLaunchKernelGGL(mi_grad_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, x, y, table, g, dx, dy, n_pix, (long)C,
                           per_image ? 1 : 0, b);
    else
        hipLaunchKernelGGL(mi_grad_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, x, y, table, g, dx, dy, n_pix, (long)C,
                           per_image ? 1 : 0, b);
    return check_launch("mi_bwd");
}
