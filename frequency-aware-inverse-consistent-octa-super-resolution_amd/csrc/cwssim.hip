// Complex-wavelet structural similarity (CW-SSIM; Wang & Simoncelli 2005, Sampat et al. 2009), fp32: for two complex bands cx, cy
// of one level as contiguous (P, h, w, 2) tensors, P = N * C * 6 planes, and a win x win box window at every valid position p
// ((h - win + 1) x (w - win + 1) positions, no padding)
//
//   z_p = sum_{q in W(p)} cx_q conj(cy_q)     E_p = sum_W |cx_q|^2 + sum_W |cy_q|^2     S_p = (2 |z_p| + K) / (E_p + K)
//
// and its gradient with u_p = z_p / |z_p| (0 where |z_p| = 0), a_p = 2 / (E_p + K), b_p = 2 S_p / (E_p + K):
//
//   A_q = sum_{p: q in W(p)} a_p u_p     B_q = sum_{p: q in W(p)} b_p     dS/dcx_q = cy_q A_q - cx_q B_q     dS/dcy_q = cx_q conj(A_q) - cy_q B_q
//
// cwssim_index: a block takes a 16 x 64 tile of positions of one plane, stages the tile plus a halo of win - 1 rows and columns of
//   both bands into LDS as four product planes (z real, z imaginary, |cx|^2, |cy|^2), box-sums them separably (rows, then
//   columns), forms S_p, writes one partial sum per block and, where the map pointers are not null, a_p u_p and b_p per position.
// cwssim_grad: a block takes a 16 x 64 tile of coefficients, stages the maps of the positions whose windows reach the tile (zero
//   outside the valid positions), box-sums them the same way into A_q, B_q and writes gx and / or gy, scaled by
//   gscale[n] / count_image: the upstream gradient is read on the device.
// cwssim_final: one block adds every image's partials (contiguous: the blocks are plane-major) in double in a fixed order.
//
// Exactness.  cw_prod is the only place a product of two coefficients is formed -- z = cw_prod(cx, cy), |c|^2 = cw_prod(c, c).x --
// and the file is compiled without contraction, so for cx == cy the imaginary part is exactly 0, z real equals both |c|^2 sums
// bit for bit, S_p == 1, a_p u_p == (b_p, 0) and both gradients are exactly 0; swapping the bands conjugates z exactly, so
// S(x, y) == S(y, x) and the gradients swap.  Every box sum runs in a fixed order; no atomics, no state, nothing allocated.
#include "common.h"

#pragma clang fp contract(off)

namespace faoctasr {

constexpr int CW_TH = 16, CW_TW = 64;             // a block's tile: rows x columns; a thread owns 4 rows of one column
constexpr int CW_MAXWIN = 11;
constexpr int CW_PR = CW_TH + CW_MAXWIN - 1;      // 26 staged rows
constexpr int CW_PC = CW_TW + CW_MAXWIN - 1;      // 74 staged columns

// (re re' + im im', im re' - re im') = a conj(b)
__device__ __forceinline__ float2 cw_prod(float2 a, float2 b) {
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// a b
__device__ __forceinline__ float2 cw_mul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// out[k][i] = sum_{s < win} sum_{t < win} in[k][4 g + i + s][c + t] for the thread's column c = tid & 63 and rows 4 g + i, g = tid >> 6:
// rows first (t ascending) into mid, then columns (s ascending).  in holds rows x (64 + win - 1) values.
template <int NP>
__device__ __forceinline__ void cw_box(float (*in)[CW_PR][CW_PC], float (*mid)[CW_PR][CW_TW], int win, float out[NP][4]) {
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int rows = CW_TH + win - 1;
    __syncthreads();
    for (int r = g; r < rows; r += 4) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float s = 0.f;
            for (int t = 0; t < win; ++t) s += in[k][r][c + t];
            mid[k][r][c] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
            for (int t = 0; t < win; ++t) s += mid[k][4 * g + i + t][c];
            out[k][i] = s;
        }
    }
}

__global__ __launch_bounds__(256) void cwssim_index_kernel(const float2* __restrict__ cx, const float2* __restrict__ cy,
                                                           float2* __restrict__ map_a, float* __restrict__ map_b, float* __restrict__ part,
                                                           int h, int w, int win, float K, int tiles_h, int tiles_w) {
    __shared__ float in[4][CW_PR][CW_PC];
    __shared__ float mid[4][CW_PR][CW_TW];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const PlaneTile t = plane_tile<CW_TH, CW_TW>(tiles_h, tiles_w);
    const long plane = t.plane;
    const int ph = h - win + 1, pw = w - win + 1;
    const int rows = CW_TH + win - 1, cols = CW_TW + win - 1;
    const float2* px = cx + plane * h * (long)w;
    const float2* py = cy + plane * h * (long)w;
    for (int r = tid >> 6; r < rows; r += 4) {
        const int gi = t.y0 + r;
        for (int c = tid & 63; c < cols; c += 64) {
            const int gj = t.x0 + c;
            float2 a = make_float2(0.f, 0.f), b = a;
            if (gi < h && gj < w) {
                a = px[(long)gi * w + gj];
                b = py[(long)gi * w + gj];
            }
            const float2 z = cw_prod(a, b);
            in[0][r][c] = z.x;
            in[1][r][c] = z.y;
            in[2][r][c] = cw_prod(a, a).x;
            in[3][r][c] = cw_prod(b, b).x;
        }
    }
    float v[4][4];
    cw_box<4>(in, mid, win, v);

    float acc = 0.f;
    const int pj = t.x0 + (tid & 63);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pi = t.y0 + 4 * (tid >> 6) + i;
        if (pi < ph && pj < pw) {
            const float zr = v[0][i], zi = v[1][i];
            const float m = zi == 0.f ? fabsf(zr) : sqrtf(zr * zr + zi * zi);     // a real z: no rounding, no underflow
            const float d = (v[2][i] + v[3][i]) + K;
            const float S = (2.f * m + K) / d;
            acc += S;
            if (map_a) {
                const float a = 2.f / d;
                const long at = (plane * ph + pi) * (long)pw + pj;
                map_a[at] = m > 0.f ? make_float2(a * (zr / m), a * (zi / m)) : make_float2(0.f, 0.f);
                map_b[at] = (2.f * S) / d;
            }
        }
    }
    block_partial_store_256(acc, red, part);
}

__global__ __launch_bounds__(256) void cwssim_grad_kernel(const float2* __restrict__ cx, const float2* __restrict__ cy,
                                                          const float2* __restrict__ map_a, const float* __restrict__ map_b,
                                                          float2* __restrict__ gx, float2* __restrict__ gy, const float* __restrict__ gscale,
                                                          double count, long planes_per_image, int h, int w, int win, int tiles_h,
                                                          int tiles_w) {
    __shared__ float in[3][CW_PR][CW_PC];
    __shared__ float mid[3][CW_PR][CW_TW];
    const int tid = threadIdx.x;
    const PlaneTile t = plane_tile<CW_TH, CW_TW>(tiles_h, tiles_w);
    const long plane = t.plane;
    const int ph = h - win + 1, pw = w - win + 1;
    const int rows = CW_TH + win - 1, cols = CW_TW + win - 1;
    const float2* pa = map_a + plane * ph * (long)pw;
    const float* pb = map_b + plane * ph * (long)pw;
    for (int r = tid >> 6; r < rows; r += 4) {
        const int pi = t.y0 - (win - 1) + r;                              // the windows p = q - win + 1 .. q contain q
        for (int c = tid & 63; c < cols; c += 64) {
            const int pj = t.x0 - (win - 1) + c;
            float2 a = make_float2(0.f, 0.f);
            float b = 0.f;
            if (pi >= 0 && pi < ph && pj >= 0 && pj < pw) {
                a = pa[(long)pi * pw + pj];
                b = pb[(long)pi * pw + pj];
            }
            in[0][r][c] = a.x;
            in[1][r][c] = a.y;
            in[2][r][c] = b;
        }
    }
    float v[3][4];
    cw_box<3>(in, mid, win, v);

    const float s = (float)((double)gscale[plane / planes_per_image] / count);
    const int qj = t.x0 + (tid & 63);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qi = t.y0 + 4 * (tid >> 6) + i;
        if (qi < h && qj < w) {
            const long at = (plane * h + qi) * (long)w + qj;
            const float2 x = cx[at], y = cy[at];
            const float B = v[2][i];
            if (gx) {
                const float2 p = cw_mul(y, make_float2(v[0][i], v[1][i]));
                gx[at] = make_float2((p.x - x.x * B) * s, (p.y - x.y * B) * s);
            }
            if (gy) {
                const float2 p = cw_mul(x, make_float2(v[0][i], -v[1][i]));
                gy[at] = make_float2((p.x - y.x * B) * s, (p.y - y.y * B) * s);
            }
        }
    }
}

// an image's partials are contiguous.  Per image: thread t adds partials t, t + 256, ... in double, a fixed tree adds the
// threads, thread 0 divides by the image's positions; the batch mean is the mean of the images' double means.
__global__ __launch_bounds__(256) void cwssim_final_kernel(const float* __restrict__ part, long per_image, long N, double count,
                                                           float* __restrict__ out_image, float* __restrict__ out_mean) {
    __shared__ double red[256];
    double total = 0.0;
    for (long n = 0; n < N; ++n) {
        const double s = block_tree_256(strided_sum_256(part + n * per_image, per_image), red);
        if (threadIdx.x == 0) {
            const double m = s / count;
            out_image[n] = (float)m;
            total += m;
        }
    }
    if (threadIdx.x == 0) out_mean[0] = (float)(total / (double)N);
}

// the shape rules of every entry point; tiles over the positions (index, final) or over the coefficients (grad)
static int cw_shape(const char* what, long planes, int h, int w, int win, int over_positions, int* tiles_h, int* tiles_w, long* blocks) {
    if (win < 1 || win > CW_MAXWIN) return fail(FAOCTASR_EINVAL, "%s: window %d, 1..%d are built", what, win, CW_MAXWIN);
    if (planes < 1) return fail(FAOCTASR_EINVAL, "%s: %ld planes", what, planes);
    if (h < win || w < win) return fail(FAOCTASR_EINVAL, "%s: a %d x %d band holds no %d x %d window", what, h, w, win, win);
    const int rh = over_positions ? h - win + 1 : h, rw = over_positions ? w - win + 1 : w;
    if (plane_tiles(planes, rh, rw, CW_TH, CW_TW, tiles_h, tiles_w, blocks)) return FAOCTASR_OK;
    return fail(FAOCTASR_EINVAL, "%s: %ld planes of %ld tiles exceed the grid", what, planes, (long)*tiles_h * *tiles_w);
}

static int cw_images(const char* what, long N, long planes) {
    if (N < 1 || planes % N) return fail(FAOCTASR_EINVAL, "%s: %ld planes do not divide into %ld images", what, planes, N);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_cwssim_workspace_floats(long planes, int h, int w, int win) {
    int tiles_h, tiles_w;
    long blocks;
    if (cw_shape("cwssim_workspace_floats", planes, h, w, win, 1, &tiles_h, &tiles_w, &blocks)) return -1;
    return blocks;
}

extern "C" int faoctasr_cwssim_index(const float* cx, const float* cy, float* map_a, float* map_b, float* part, long planes, int h, int w,
                                     int win, float K, faoctasr_stream_t stream) {
    if (!cx || !cy || !part) return fail(FAOCTASR_EINVAL, "cwssim_index: null pointer");
    if ((map_a == nullptr) != (map_b == nullptr)) return fail(FAOCTASR_EINVAL, "cwssim_index: the two maps come together or not at all");
    if (!(K > 0.f) || !(K < INFINITY)) return fail(FAOCTASR_EINVAL, "cwssim_index: the constant K %g must be positive and finite", (double)K);
    int tiles_h, tiles_w, rc;
    long blocks;
    if ((rc = cw_shape("cwssim_index", planes, h, w, win, 1, &tiles_h, &tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(cwssim_index_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(cx),
                       reinterpret_cast<const float2*>(cy), reinterpret_cast<float2*>(map_a), map_b, part, h, w, win, K, tiles_h, tiles_w);
    return check_launch("cwssim_index");
}

extern "C" int faoctasr_cwssim_grad(const float* cx, const float* cy, const float* map_a, const float* map_b, float* gx, float* gy,
                                    const float* gscale, long N, long planes, int h, int w, int win, faoctasr_stream_t stream) {
    if (!cx || !cy || !map_a || !map_b || !gscale) return fail(FAOCTASR_EINVAL, "cwssim_grad: null pointer");
    if (!gx && !gy) return fail(FAOCTASR_EINVAL, "cwssim_grad: neither gradient is asked for");
    int tiles_h, tiles_w, rc;
    long blocks;
    if ((rc = cw_shape("cwssim_grad", planes, h, w, win, 0, &tiles_h, &tiles_w, &blocks))) return rc;
    if ((rc = cw_images("cwssim_grad", N, planes))) return rc;
    const long per_image = planes / N;
    const double count = (double)per_image * (double)(h - win + 1) * (double)(w - win + 1);
    hipLaunchKernelGGL(cwssim_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(cx),
                       reinterpret_cast<const float2*>(cy), reinterpret_cast<const float2*>(map_a), map_b, reinterpret_cast<float2*>(gx),
                       reinterpret_cast<float2*>(gy), gscale, count, per_image, h, w, win, tiles_h, tiles_w);
    return check_launch("cwssim_grad");
}

extern "C" int faoctasr_cwssim_final(const float* part, long N, long planes, int h, int w, int win, float* out_image, float* out_mean,
                                     faoctasr_stream_t stream) {
    if (!part || !out_image || !out_mean) return fail(FAOCTASR_EINVAL, "cwssim_final: null pointer");
    int tiles_h, tiles_w, rc;
    long blocks;
    if ((rc = cw_shape("cwssim_final", planes, h, w, win, 1, &tiles_h, &tiles_w, &blocks))) return rc;
    if ((rc = cw_images("cwssim_final", N, planes))) return rc;
    const long per_image = planes / N;
    const double count = (double)per_image * (double)(h - win + 1) * (double)(w - win + 1);
    hipLaunchKernelGGL(cwssim_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, blocks / N, N, count, out_image, out_mean);
    return check_launch("cwssim_final");
}
