// Total-variation loss (model.py:17-33 of the reference; train.py:178) for x[B,C,H,W], fp32:
//
//   L = weight * 2 * ( S_h / count_h + S_w / count_w ) / B        S_h = sum (x[.,.,i+1,j] - x[.,.,i,j])^2,  count_h = C (H-1) W
//                                                                  S_w = sum (x[.,.,i,j+1] - x[.,.,i,j])^2,  count_w = C H (W-1)
//
// Forward, two launches.  A thread owns TV_ROWS rows of one group of V adjacent columns (V = 4: one float4 per row, when W % 4 == 0
// and x is 16-byte aligned; V = 1 otherwise) of one (sample, channel) plane and walks down them: the row above stays in its
// registers, so a vertical difference costs no second load; the column right of its group comes from the next lane
// (__shfl_down).  Only the last lane of a wave whose row goes on in the next wave loads that one float itself, and the row below
// a strip is loaded by the strip's threads and by the next strip's: 1/TV_ROWS of the image is requested twice, the second time out
// of L2.  S_h and S_w are kept apart (they have different divisors), summed over the block in a fixed order and stored as one
// pair of partials per block; a single-block kernel adds the partials in a fixed order in double, applies the divisors in the
// reference's order (weight * 2 * (..) / B) and writes one float.  No atomics: the loss is bit-reproducible.
//
// Backward, one launch over the same thread layout:
//   dx[i,j] = g * weight*2/B * ( 2/count_h * ((x[i,j]-x[i-1,j]) [i>0] - (x[i+1,j]-x[i,j]) [i<H-1])
//                              + 2/count_w * ((x[i,j]-x[i,j-1]) [j>0] - (x[i,j+1]-x[i,j]) [j<W-1]) )
// with g read from device memory (no host read: the op is capturable).
#include <cstdint>
#include "common.h"

namespace faoctasr {

constexpr int TV_ROWS = 8;

template <int V>
__device__ __forceinline__ void tv_load(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

// work item q -> (plane, strip of TV_ROWS rows, group of V columns); consecutive lanes hold consecutive column groups of one row
struct TvItem {
    bool active;
    int r0, c0;
    long row0;          // index of x[plane, r0, c0]
};

template <int V>
__device__ __forceinline__ TvItem tv_item(long items, int H, int W, int strips) {
    TvItem it;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    it.active = q < items;
    const long qq = it.active ? q : 0;
    const int WV = W / V;
    const int cv = (int)(qq % WV);
    const long t = qq / WV;
    it.r0 = (int)(t % strips) * TV_ROWS;
    it.c0 = cv * V;
    it.row0 = ((t / strips) * H + it.r0) * (long)W + it.c0;
    return it;
}

template <int V>
__global__ __launch_bounds__(256) void tv_fwd_kernel(const float* __restrict__ x, float* __restrict__ part, long items, int H, int W,
                                                     int strips) {
    __shared__ float red[4];
    const TvItem it = tv_item<V>(items, H, W, strips);
    const float* base = x + it.row0;
    const bool has_right = it.c0 + V < W;
    const int lane = threadIdx.x & 63;
    float prev[V], cur[V];
#pragma unroll
    for (int k = 0; k < V; ++k) prev[k] = cur[k] = 0.f;
    float sh = 0.f, sw = 0.f;
#pragma unroll
    for (int r = 0; r <= TV_ROWS; ++r) {               // row r0 + TV_ROWS belongs to the next strip: read for its vertical difference only
        const bool ok = it.active && it.r0 + r < H;
        if (ok) tv_load<V>(base + (long)r * W, cur);
        if (r < TV_ROWS) {
            float right = __shfl_down(cur[0], 1, 64);
            if (ok && has_right && lane == 63) right = base[(long)r * W + V];
            if (ok) {
#pragma unroll
                for (int k = 0; k + 1 < V; ++k) { const float d = cur[k + 1] - cur[k]; sw += d * d; }
                if (has_right) { const float d = right - cur[V - 1]; sw += d * d; }
            }
        }
        if (r > 0 && ok) {
#pragma unroll
            for (int k = 0; k < V; ++k) { const float d = cur[k] - prev[k]; sh += d * d; }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) prev[k] = cur[k];
    }
    sh = block_sum_256(sh, red);
    sw = block_sum_256(sw, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sh;
        part[(long)gridDim.x + blockIdx.x] = sw;
    }
}

// part[0, np): the blocks' S_h, part[np, 2 np): their S_w.  Thread t adds partials t, t + 256, ... in double, then a fixed tree.
__global__ __launch_bounds__(256) void tv_final_kernel(const float* __restrict__ part, long np, float* __restrict__ out, double count_h,
                                                       double count_w, double weight2, double batch) {
    __shared__ double red_h[256], red_w[256];
    double a = 0.0, b = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) { a += (double)part[i]; b += (double)part[np + i]; }
    red_h[threadIdx.x] = a;
    red_w[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { red_h[threadIdx.x] += red_h[threadIdx.x + o]; red_w[threadIdx.x] += red_w[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(weight2 * (red_h[0] / count_h + red_w[0] / count_w) / batch);
}

template <int V>
__global__ __launch_bounds__(256) void tv_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ dx,
                                                     long items, int H, int W, int strips, float kh, float kw) {
    const TvItem it = tv_item<V>(items, H, W, strips);
    const float* base = x + it.row0;
    float* out = dx + it.row0;
    const bool has_left = it.c0 > 0, has_right = it.c0 + V < W;
    const int lane = threadIdx.x & 63;
    const float gs = g[0];
    const float ch = gs * kh, cw = gs * kw;
    float up[V], cur[V], dn[V];
#pragma unroll
    for (int k = 0; k < V; ++k) up[k] = cur[k] = dn[k] = 0.f;
    if (it.active && it.r0 > 0) tv_load<V>(base - W, up);
    if (it.active) tv_load<V>(base, cur);               // strips = ceil(H / TV_ROWS): row r0 exists
#pragma unroll
    for (int r = 0; r < TV_ROWS; ++r) {
        const int row = it.r0 + r;
        const bool ok = it.active && row < H;
        const bool has_dn = ok && row + 1 < H;
        if (has_dn) tv_load<V>(base + (long)(r + 1) * W, dn);
        float left = __shfl_up(cur[V - 1], 1, 64), right = __shfl_down(cur[0], 1, 64);
        if (ok && has_left && lane == 0) left = base[(long)r * W - 1];
        if (ok && has_right && lane == 63) right = base[(long)r * W + V];
        if (ok) {
            float d[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float xv = cur[k];
                float a = 0.f, b = 0.f;
                if (row > 0) a += xv - up[k];
                if (has_dn) a -= dn[k] - xv;
                const float l = k > 0 ? cur[k - 1] : left, rr = k + 1 < V ? cur[k + 1] : right;
                if (k > 0 || has_left) b += xv - l;
                if (k + 1 < V || has_right) b -= rr - xv;
                d[k] = ch * a + cw * b;
            }
            if constexpr (V == 4) *reinterpret_cast<float4*>(out + (long)r * W) = make_float4(d[0], d[1], d[2], d[3]);
            else out[(long)r * W] = d[0];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) { up[k] = cur[k]; cur[k] = dn[k]; }
    }
}

struct TvGeom {
    int V, strips;
    long items, blocks;
};

// V = 4 needs every row start 16-byte aligned: W % 4 == 0 and aligned base pointers (NULL counts as aligned: the workspace query)
static TvGeom tv_geom(const void* x, const void* dx, int B, int C, int H, int W) {
    TvGeom t;
    t.V = (W % 4 == 0 && (((uintptr_t)x | (uintptr_t)dx) & 15) == 0) ? 4 : 1;
    t.strips = (H + TV_ROWS - 1) / TV_ROWS;
    t.items = (long)B * C * t.strips * (W / t.V);
    t.blocks = (t.items + 255) / 256;
    return t;
}

static int tv_check(const char* what, int B, int C, int H, int W) {
    if (B < 1 || C < 1 || H < 2 || W < 2) return fail(FAOCTASR_EINVAL, "%s: bad shape B %d C %d H %d W %d (H, W >= 2)", what, B, C, H, W);
    if ((long)B * C * ((H + TV_ROWS - 1) / TV_ROWS) * W > 0x7fffffffL * 256) return fail(FAOCTASR_EUNSUPPORTED, "%s: B %d C %d H %d W %d needs more than 2^31 - 1 blocks", what, B, C, H, W);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_tv_loss_workspace_floats(int B, int C, int H, int W) {
    if (tv_check("tv_loss_workspace_floats", B, C, H, W)) return -1;
    const long items = (long)B * C * ((H + TV_ROWS - 1) / TV_ROWS) * W;      // the scalar path's block count bounds the vector path's
    return 2 * ((items + 255) / 256);
}

extern "C" int faoctasr_tv_loss_fwd(const float* x, float* out, float* workspace, int B, int C, int H, int W, float weight,
                                    faoctasr_stream_t stream) {
    if (!x || !out || !workspace) return fail(FAOCTASR_EINVAL, "tv_loss_fwd: null pointer");
    int rc = tv_check("tv_loss_fwd", B, C, H, W);
    if (rc) return rc;
    const TvGeom t = tv_geom(x, nullptr, B, C, H, W);
    if (t.V == 4)
        hipLaunchKernelGGL(tv_fwd_kernel<4>, dim3((unsigned)t.blocks), dim3(256), 0, (hipStream_t)stream, x, workspace, t.items, H, W, t.strips);
    else
        hipLaunchKernelGGL(tv_fwd_kernel<1>, dim3((unsigned)t.blocks), dim3(256), 0, (hipStream_t)stream, x, workspace, t.items, H, W, t.strips);
    rc = check_launch("tv_loss_fwd (partial sums)");
    if (rc) return rc;
    hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, t.blocks, out,
                       (double)C * (H - 1) * W, (double)C * H * (W - 1), 2.0 * (double)weight, (double)B);
    return check_launch("tv_loss_fwd (final)");
}

extern "C" int faoctasr_tv_loss_bwd(const float* x, const float* g, float* dx, int B, int C, int H, int W, float weight,
                                    faoctasr_stream_t stream) {
    if (!x || !g || !dx) return fail(FAOCTASR_EINVAL, "tv_loss_bwd: null pointer");
    int rc = tv_check("tv_loss_bwd", B, C, H, W);
    if (rc) return rc;
    const TvGeom t = tv_geom(x, dx, B, C, H, W);
    const double s = 2.0 * (double)weight / (double)B;
    const float kh = (float)(s * 2.0 / ((double)C * (H - 1) * W)), kw = (float)(s * 2.0 / ((double)C * H * (W - 1)));
    if (t.V == 4)
        hipLaunchKernelGGL(tv_bwd_kernel<4>, dim3((unsigned)t.blocks), dim3(256), 0, (hipStream_t)stream, x, g, dx, t.items, H, W, t.strips, kh, kw);
    else
        hipLaunchKernelGGL(tv_bwd_kernel<1>, dim3((unsigned)t.blocks), dim3(256), 0, (hipStream_t)stream, x, g, dx, t.items, H, W, t.strips, kh, kw);
    return check_launch("tv_loss_bwd");
}
