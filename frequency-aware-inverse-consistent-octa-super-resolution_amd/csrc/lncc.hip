// Local (windowed) normalised cross-correlation, LNCC, fp32.  For a pair a, b of (N, C, H, W), an odd window side win in 3..15,
// n = win^2, r = win / 2 and eps > 0, with box(t)_p the sum of t over the win x win window centred on p (samples beyond the image 0):
//
//   Sa = box(a)   Sb = box(b)   Saa = box(a a)   Sbb = box(b b)   Sab = box(a b)
//   u = Sab - Sa Sb / n    va = Saa - Sa Sa / n    vb = Sbb - Sb Sb / n    D = va vb + eps
//   cc_p = u^2 / D,   LNCC[n] = the mean of cc_p over c, y, x
//
// lncc_index<WIN>: a block takes a 16 x 32 tile of one plane, stages the tile plus a halo of r of both images straight from a, b into
//   LDS, forms the five sums separably (rows, then columns) and writes ONE partial sum of cc_p per block (per-thread sum, 64-lane
//   butterfly, the four waves in a fixed order: no atomics).
// lncc_final: one block adds an image's partials in double in a fixed order, writes the scores, their mean and, when asked, the table
//   fac[n] = 1 / (C H W) (times 1 / N when averaging), so the backward reads nothing on the host.
// lncc_grad<WIN>: a block takes a 16 x 16 tile, recomputes the five sums on the tile plus r from a staged halo of 2 r, forms there the
//   cotangent maps
//     dSab = 2 u / D,  dSaa = -u^2 vb / D^2,  dSa = -((2 u / D) Sb + 2 dSaa Sa) / n   and the mirror images dSbb, dSb,
//   zero beyond the image, box-sums them (the box is its own transpose) and writes
//     da_q = box(dSa)_q + 2 a_q box(dSaa)_q + b_q box(dSab)_q,
//   times fac[n] and the upstream gradient read on the device.  A null da / db skips that side's maps, sums and stores.
//
// The passes.  Every box pass keeps a strip of consecutive outputs of one thread in registers: a row pass reads the win + 3 samples
// under four neighbouring outputs once (the row strides are multiples of four floats, so the reads are wide) and a column pass the
// win + 1 rows under two; every window sum is a direct sum of its win terms in index order -- no sliding add / subtract, whose
// rounding would grow along the strip.
//
// Exactness.  The file is compiled without contraction.  The products of the two images (ln_prod), the statistics (ln_stat) and the
// cotangents (ln_cot) are symmetric in the two sides, and both sides' sums run in one order: swapping a and b leaves the score bit for
// bit and swaps the gradients.  The upstream gradient enters as one factor of the last product, so halving it halves da.  Every sum
// runs in a fixed order; nothing is allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int LN_MAX_WIN = 15;
constexpr int LF_TY = 16, LF_TX = 32;                // the tile of lncc_index
constexpr int LB_T = 16;                             // the tile of lncc_grad (square)
constexpr int LF_PS = 96;                            // lncc_index: row stride of the staged images, = 32 (mod 64) floats: eight 16-byte strip
                                                     // reads of each of four neighbouring rows fall on 16 different 16-byte bank slots

constexpr int ln_up4(int v) { return (v + 3) / 4 * 4; }

// the five statistics of a sample, in the order a, b, a a, b b, a b: the one place where the two images meet
__device__ __forceinline__ void ln_prod(float a, float b, float (&t)[5]) {
    t[0] = a; t[1] = b; t[2] = a * a; t[3] = b * b; t[4] = a * b;
}

// Row pass of the statistics: the five window sums of four neighbouring outputs from the WIN + 3 samples under them, pa and pb at the
// first sample of the first window
template <int WIN>
__device__ __forceinline__ void ln_row_stats(const float* __restrict__ pa, const float* __restrict__ pb, float (&s)[4][5]) {
    float a[WIN + 3], b[WIN + 3];
#pragma unroll
    for (int k = 0; k < WIN + 3; ++k) { a[k] = pa[k]; b[k] = pb[k]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ln_prod(a[j], b[j], s[j]);
#pragma unroll
        for (int k = 1; k < WIN; ++k) {
            float t[5];
            ln_prod(a[j + k], b[j + k], t);
#pragma unroll
            for (int m = 0; m < 5; ++m) s[j][m] += t[m];
        }
    }
}

// Row pass of one map: the window sums of four neighbouring outputs
template <int WIN>
__device__ __forceinline__ void ln_row_box(const float* __restrict__ p, float (&s)[4]) {
    float v[WIN + 3];
#pragma unroll
    for (int k = 0; k < WIN + 3; ++k) v[k] = p[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = v[j];
#pragma unroll
        for (int k = 1; k < WIN; ++k) s[j] += v[j + k];
    }
}

// Column pass of one map: the window sums of two outputs, one under the other, from the WIN + 1 rows under them
template <int WIN>
__device__ __forceinline__ void ln_col_box(const float* __restrict__ p, int stride, float (&s)[2]) {
    float v[WIN + 1];
#pragma unroll
    for (int k = 0; k < WIN + 1; ++k) v[k] = p[k * stride];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        s[j] = v[j];
#pragma unroll
        for (int k = 1; k < WIN; ++k) s[j] += v[j + k];
    }
}

// u, va, vb, D of one position; symmetric: the sides exchanged give the same u and D and va, vb exchanged
struct LnStat { float u, va, vb, D; };
__device__ __forceinline__ LnStat ln_stat(const float (&s)[5], float n, float eps) {
    LnStat c;
    c.u = s[4] - (s[0] * s[1]) / n;
    c.va = s[2] - (s[0] * s[0]) / n;
    c.vb = s[3] - (s[1] * s[1]) / n;
    c.D = c.va * c.vb + eps;
    return c;
}

// the cotangents of the five sums at one position (of cc_p, upstream 1), in the order dSa, dSaa, dSab, dSb, dSbb
__device__ __forceinline__ void ln_cot(const float (&s)[5], float n, float eps, float (&d)[5]) {
    const LnStat c = ln_stat(s, n, eps);
    const float cu = (2.f * c.u) / c.D;
    const float q = (c.u * c.u) / (c.D * c.D);
    const float ca = -(q * c.vb), cb = -(q * c.va);
    d[2] = cu;
    d[1] = ca;
    d[4] = cb;
    d[0] = -((cu * s[1] + (2.f * ca) * s[0]) / n);
    d[3] = -((cu * s[0] + (2.f * cb) * s[1]) / n);
}

// Stage ROWS x COLS values of both images from (gy0, gx0), zero beyond the image, into two arrays of row stride PS
template <int ROWS, int COLS, int PS>
__device__ __forceinline__ void ln_stage(const float* __restrict__ ap, const float* __restrict__ bp, int H, int W, int gy0, int gx0,
                                         float* __restrict__ sa, float* __restrict__ sb) {
    for (int i = threadIdx.x; i < ROWS * COLS; i += 256) {
        const int r = i / COLS, c = i - r * COLS;
        const int gy = gy0 + r, gx = gx0 + c;
        const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        const long off = (long)gy * W + gx;
        sa[r * PS + c] = in ? ap[off] : 0.f;
        sb[r * PS + c] = in ? bp[off] : 0.f;
    }
}

template <int WIN>
__global__ __launch_bounds__(256) void lncc_index_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ part, int H,
                                                         int W, int tiles_h, int tiles_w, float eps) {
    constexpr int R = WIN / 2, PY = LF_TY + 2 * R;
    constexpr int PC = LF_TX - 4 + ln_up4(WIN + 3);         // staged columns: the tile, the halo and what the last strip's wide reads touch
    static_assert(PC <= LF_PS && PC >= LF_TX + 2 * R, "staged row");
    static_assert(PY * (LF_TX / 4) <= 256, "one row strip per thread");
    __shared__ __attribute__((aligned(16))) float st[2][PY * LF_PS];
    __shared__ __attribute__((aligned(16))) float hs[5][PY * LF_TX];
    __shared__ float red[4];
    const PlaneTile t = plane_tile<LF_TY, LF_TX>(tiles_h, tiles_w);
    const long plane_off = (long)t.plane * H * W;
    ln_stage<PY, PC, LF_PS>(a + plane_off, b + plane_off, H, W, t.y0 - R, t.x0 - R, st[0], st[1]);
    __syncthreads();
    if (threadIdx.x < PY * (LF_TX / 4)) {
        const int r = threadIdx.x >> 3, s4 = 4 * (threadIdx.x & 7);
        float s[4][5];
        ln_row_stats<WIN>(st[0] + r * LF_PS + s4, st[1] + r * LF_PS + s4, s);
#pragma unroll
        for (int m = 0; m < 5; ++m)
            *reinterpret_cast<float4*>(hs[m] + r * LF_TX + s4) = make_float4(s[0][m], s[1][m], s[2][m], s[3][m]);
    }
    __syncthreads();
    const int col = threadIdx.x & 31, r0 = 2 * (threadIdx.x >> 5);
    float s[5][2];
#pragma unroll
    for (int m = 0; m < 5; ++m) ln_col_box<WIN>(hs[m] + r0 * LF_TX + col, LF_TX, s[m]);
    const float n = (float)(WIN * WIN);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (t.y0 + r0 + j < H && t.x0 + col < W) {
            const float v[5] = {s[0][j], s[1][j], s[2][j], s[3][j], s[4][j]};
            const LnStat c = ln_stat(v, n, eps);
            acc += (c.u * c.u) / c.D;
        }
    }
    block_partial_store_256(acc, red, part);
}

__global__ __launch_bounds__(256) void lncc_final_kernel(const float* __restrict__ ws, int per_image, int N, double count, int average,
                                                         float* __restrict__ out_image, float* __restrict__ out_mean, float* __restrict__ fac) {
    __shared__ double red[256];
    double total = 0.0;
    for (int n = 0; n < N; ++n) {
        const double sum = block_tree_256(strided_sum_256(ws + (long)n * per_image, per_image), red);
        if (threadIdx.x == 0) {
            const double score = sum / count;
            out_image[n] = (float)score;
            total += score;
            if (fac) fac[n] = (float)((average ? 1.0 / (double)N : 1.0) / count);
        }
    }
    if (threadIdx.x == 0) out_mean[0] = (float)(total / (double)N);
}

template <int WIN>
__global__ __launch_bounds__(256) void lncc_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ fac,
                                                        const float* __restrict__ gout, int gN, float* __restrict__ da, float* __restrict__ db,
                                                        int C, int H, int W, int tiles_h, int tiles_w, float eps) {
    constexpr int R = WIN / 2, T = LB_T;
    constexpr int Q = T + 2 * R;                         // the cotangent region: the tile plus r
    constexpr int P = T + 4 * R;                         // the staged region: the tile plus 2 r
    constexpr int NS = (Q + 3) / 4, QS = 4 * NS;         // row strips of the cotangent region; row stride of its maps
    constexpr int PC = QS - 4 + ln_up4(WIN + 3);         // staged columns, with what the last strip's wide reads touch; also the row stride
    static_assert(PC >= P && PC % 4 == 0, "staged row");
    static_assert(Q % 2 == 0 && 12 + WIN + 3 <= QS, "cotangent maps");
    static_assert(6 * Q * T <= 5 * P * QS, "the box sums of the maps fit the row sums they replace");
    static_assert(2 * Q * (T / 4) <= 256, "one map strip per thread");
    __shared__ __attribute__((aligned(16))) float st[2][P * PC];
    __shared__ __attribute__((aligned(16))) float hs[5][P * QS];      // row sums of the statistics; later bx: [side][map][Q x T]
    __shared__ __attribute__((aligned(16))) float mp[5][Q * QS];      // dSa, dSaa, dSab, dSb, dSbb
    const PlaneTile t = plane_tile<T, T>(tiles_h, tiles_w);
    const long plane_off = (long)t.plane * H * W;
    const bool wa = da != nullptr, wb = db != nullptr;   // uniform: a side that is not asked for costs no map, no sum, no store
    ln_stage<P, PC, PC>(a + plane_off, b + plane_off, H, W, t.y0 - 2 * R, t.x0 - 2 * R, st[0], st[1]);
    __syncthreads();
    for (int it = threadIdx.x; it < P * NS; it += 256) {
        const int r = it / NS, s4 = 4 * (it - r * NS);
        float s[4][5];
        ln_row_stats<WIN>(st[0] + r * PC + s4, st[1] + r * PC + s4, s);
#pragma unroll
        for (int m = 0; m < 5; ++m)
            *reinterpret_cast<float4*>(hs[m] + r * QS + s4) = make_float4(s[0][m], s[1][m], s[2][m], s[3][m]);
    }
    __syncthreads();
    const float n = (float)(WIN * WIN);
    for (int it = threadIdx.x; it < (Q / 2) * QS; it += 256) {
        const int rp = it / QS, col = it - rp * QS, r0 = 2 * rp;
        float s[5][2];
#pragma unroll
        for (int m = 0; m < 5; ++m) ln_col_box<WIN>(hs[m] + r0 * QS + col, QS, s[m]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = t.y0 - R + r0 + j, gx = t.x0 - R + col;
            float d[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (col < Q && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
                const float v[5] = {s[0][j], s[1][j], s[2][j], s[3][j], s[4][j]};
                ln_cot(v, n, eps, d);
            }
            const int at = (r0 + j) * QS + col;
            mp[2][at] = d[2];
            if (wa) { mp[0][at] = d[0]; mp[1][at] = d[1]; }
            if (wb) { mp[3][at] = d[3]; mp[4][at] = d[4]; }
        }
    }
    __syncthreads();                                     // the row sums are dead from here: hs takes the maps' row sums
    float* bx = hs[0];
    if (threadIdx.x < 2 * Q * (T / 4)) {
        const int side = threadIdx.x / (Q * (T / 4)), rem = threadIdx.x - side * (Q * (T / 4));
        const int r = rem >> 2, s4 = 4 * (rem & 3);
        if (side ? wb : wa) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const float* src = m == 2 ? mp[2] : mp[3 * side + m];
                float s[4];
                ln_row_box<WIN>(src + r * QS + s4, s);
                *reinterpret_cast<float4*>(bx + (3 * side + m) * (Q * T) + r * T + s4) = make_float4(s[0], s[1], s[2], s[3]);
            }
        }
    }
    __syncthreads();
    const int side = threadIdx.x >> 7, col = threadIdx.x & 15, r0 = 2 * ((threadIdx.x >> 4) & 7);
    float* __restrict__ out = side ? db : da;
    if (out != nullptr) {
        float s[3][2];
#pragma unroll
        for (int m = 0; m < 3; ++m) ln_col_box<WIN>(bx + (3 * side + m) * (Q * T) + r0 * T + col, T, s[m]);
        const float gv = fac[t.plane / C] * gout[gN > 1 ? t.plane / C : 0];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gy = t.y0 + r0 + j, gx = t.x0 + col;
            if (gy < H && gx < W) {
                const int at = (2 * R + r0 + j) * PC + 2 * R + col;
                const float own = st[side][at], other = st[1 - side][at];
                const float d = (s[0][j] + (2.f * own) * s[1][j]) + other * s[2][j];
                out[plane_off + (long)gy * W + gx] = gv * d;
            }
        }
    }
}

static int ln_shape(const char* what, long planes, int H, int W) {
    if (planes < 1 || H < 1 || W < 1) return fail(FAOCTASR_EINVAL, "%s: bad shape (%ld planes of %d x %d)", what, planes, H, W);
    if ((long)H * W > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: a plane of %d x %d exceeds 2^31 - 1 samples", what, H, W);
    return FAOCTASR_OK;
}

static int ln_consts(const char* what, int win, float eps) {
    if (win < 3 || win > LN_MAX_WIN || win % 2 == 0) return fail(FAOCTASR_EINVAL, "%s: win %d must be odd in 3..%d", what, win, LN_MAX_WIN);
    if (!(eps > 0.f) || !(eps < INFINITY)) return fail(FAOCTASR_EINVAL, "%s: eps %g must be positive and finite", what, (double)eps);
    return FAOCTASR_OK;
}

static int ln_tiles(const char* what, long planes, int H, int W, int TY, int TX, int* tiles_h, int* tiles_w, long* blocks) {
    if (plane_tiles(planes, H, W, TY, TX, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EUNSUPPORTED, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

// one instantiation per odd window side
#define LN_DISPATCH(win, CALL) \
    switch (win) {             \
        case 3: CALL(3); break;   \
        case 5: CALL(5); break;   \
        case 7: CALL(7); break;   \
        case 9: CALL(9); break;   \
        case 11: CALL(11); break; \
        case 13: CALL(13); break; \
        default: CALL(15); break; \
    }

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_lncc_workspace_floats(long planes, int H, int W) {
    int th, tw;
    long blocks;
    if (ln_shape("lncc_workspace_floats", planes, H, W)) return -1;
    if (ln_tiles("lncc_workspace_floats", planes, H, W, LF_TY, LF_TX, &th, &tw, &blocks)) return -1;
    return blocks;
}

extern "C" int faoctasr_lncc_index(const float* a, const float* b, float* workspace, long planes, int H, int W, int win, float eps,
                                   faoctasr_stream_t stream) {
    if (!a || !b || !workspace) return fail(FAOCTASR_EINVAL, "lncc_index: null pointer");
    int rc, th, tw;
    long blocks;
    if ((rc = ln_shape("lncc_index", planes, H, W))) return rc;
    if ((rc = ln_consts("lncc_index", win, eps))) return rc;
    if ((rc = ln_tiles("lncc_index", planes, H, W, LF_TY, LF_TX, &th, &tw, &blocks))) return rc;
#define LN_INDEX(WIN) \
    hipLaunchKernelGGL(lncc_index_kernel<WIN>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, workspace, H, W, th, tw, eps)
    LN_DISPATCH(win, LN_INDEX)
#undef LN_INDEX
    return check_launch("lncc_index");
}

extern "C" int faoctasr_lncc_final(const float* workspace, long N, long C, int H, int W, int average, float* out_image, float* out_mean,
                                   float* fac, faoctasr_stream_t stream) {
    if (!workspace || !out_image || !out_mean) return fail(FAOCTASR_EINVAL, "lncc_final: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "lncc_final: bad shape (%ld images of %ld channels)", N, C);
    int rc, th, tw;
    long blocks;
    if ((rc = ln_shape("lncc_final", N * C, H, W))) return rc;
    if ((rc = ln_tiles("lncc_final", N * C, H, W, LF_TY, LF_TX, &th, &tw, &blocks))) return rc;
    hipLaunchKernelGGL(lncc_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, (int)(blocks / N), (int)N,
                       (double)C * (double)H * (double)W, average, out_image, out_mean, fac);
    return check_launch("lncc_final");
}

extern "C" int faoctasr_lncc_grad(const float* a, const float* b, const float* fac, const float* g, int gN, float* da, float* db, long N, long C,
                                  int H, int W, int win, float eps, faoctasr_stream_t stream) {
    if (!a || !b || !fac || !g) return fail(FAOCTASR_EINVAL, "lncc_grad: null pointer");
    if (N < 1 || C < 1 || N > 0x7fffffffL || C > 0x7fffffffL) return fail(FAOCTASR_EINVAL, "lncc_grad: bad shape (%ld images of %ld channels)", N, C);
    if (gN != 1 && gN != N) return fail(FAOCTASR_EINVAL, "lncc_grad: gN must be 1 or N");
    if (!da && !db) return fail(FAOCTASR_EINVAL, "lncc_grad: neither gradient is asked for");
    int rc, th, tw;
    long blocks;
    if ((rc = ln_shape("lncc_grad", N * C, H, W))) return rc;
    if ((rc = ln_consts("lncc_grad", win, eps))) return rc;
    if ((rc = ln_tiles("lncc_grad", N * C, H, W, LB_T, LB_T, &th, &tw, &blocks))) return rc;
#define LN_GRAD(WIN) \
    hipLaunchKernelGGL(lncc_grad_kernel<WIN>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, fac, g, gN, da, db, (int)C, H, W, th, tw, eps)
    LN_DISPATCH(win, LN_GRAD)
#undef LN_GRAD
    return check_launch("lncc_grad");
}
