// Shared helpers for the gfx950 kernels (error text, launch checks, activation math).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdarg>
#include "faoctasr.h"

namespace faoctasr {

char* err_buf();
int fail(int code, const char* fmt, ...);
// which kernel family the last convolution-type call of this thread was dispatched to (diagnostics: faoctasr_last_route)
enum Route { ROUTE_NONE = 0, ROUTE_GATHER_FLAT = 1, ROUTE_PATCH = 2, ROUTE_WINOGRAD = 3, ROUTE_BF16X3 = 4, ROUTE_M1_FWD = 5, ROUTE_NARROW = 6,
             ROUTE_WGRAD_FLAT = 11, ROUTE_WGRAD_PATCH = 12, ROUTE_WGRAD_S1 = 13, ROUTE_M1_WGRAD = 14, ROUTE_WGRAD_X3 = 15, ROUTE_STEM_DGRAD = 7, ROUTE_STEM_WGRAD = 16,
             ROUTE_NARROW_X2 = 8 };
void set_route(int r);
extern thread_local int g_no_split_k;
// the absmax slot faoctasr_out_absmax left for this thread's next producer call (BatchNorm forward / backward, cat2_act forward):
// taken (and cleared) by that call
extern thread_local unsigned* g_out_absmax;
unsigned* take_out_absmax();

// Opt a kernel in to more than 64 KiB of dynamic LDS.  hipFuncSetAttribute is issued once per (kernel, size step), not
// per launch: the only process-wide state of the library is this grow-only record of attributes already set
// (one process drives one GPU).
void lds_optin(const void* kernel, size_t lds_bytes);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FAOCTASR_EHIP, "%s: %s", what, hipGetErrorString(e));
    return FAOCTASR_OK;
}

__device__ __forceinline__ float act_apply(float v, int act, float slope) {
    switch (act) {
        case FAOCTASR_ACT_RELU: return v > 0.f ? v : 0.f;
        case FAOCTASR_ACT_LRELU: return v > 0.f ? v : v * slope;
        case FAOCTASR_ACT_TANH: return tanhf(v);
        default: return v;
    }
}
// derivative expressed through the activation OUTPUT y
__device__ __forceinline__ float act_grad_from_out(float y, int act, float slope) {
    switch (act) {
        case FAOCTASR_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case FAOCTASR_ACT_LRELU: return y > 0.f ? 1.f : slope;
        case FAOCTASR_ACT_TANH: return 1.f - y * y;
        default: return 1.f;
    }
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum for 256-thread blocks (float or double); result valid in every thread
template <class T>
__device__ __forceinline__ T block_sum_256(T v, T* red /* >= 4 values */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// a block's partial sum: per-thread sum -> 64-lane butterfly -> the four waves, in that order; thread 0 stores
__device__ __forceinline__ void block_partial_store_256(float v, float* red /* >= 4 floats */, float* part) {
    v = block_sum_256(v, red);                                          // ((red[0] + red[1]) + red[2]) + red[3]
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// the single-block finish of those partials, in double: thread t adds p[t], p[t + 256], ... in index order ...
template <class T>
__device__ __forceinline__ double strided_sum_256(const T* __restrict__ p, long n) {
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) a += (double)p[i];
    return a;
}

// ... and a fixed tree adds the 256 threads' values (red[t] += red[t + o], o = 128 .. 1).  Returns red[0] to every thread; the
// barrier after it lets a loop reuse red
__device__ __forceinline__ double block_tree_256(double v, double* red /* 256 doubles */) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// blockIdx.x = (plane * tiles_h + tile row) * tiles_w + tile column of TY x TX tiles: no 65535-plane limit, and a plane's
// (an image's) blocks are contiguous
struct PlaneTile { int plane, y0, x0; };
template <int TY, int TX>
__device__ __forceinline__ PlaneTile plane_tile(int tiles_h, int tiles_w) {
    unsigned bi = blockIdx.x;
    PlaneTile t;
    t.x0 = (int)(bi % (unsigned)tiles_w) * TX; bi /= (unsigned)tiles_w;
    t.y0 = (int)(bi % (unsigned)tiles_h) * TY;
    t.plane = (int)(bi / (unsigned)tiles_h);
    return t;
}

// the grid of that decode for `planes` planes of h x w; false when it passes 2^31 - 1 blocks
inline bool plane_tiles(long planes, int h, int w, int TY, int TX, int* tiles_h, int* tiles_w, long* blocks) {
    *tiles_h = (h + TY - 1) / TY;
    *tiles_w = (w + TX - 1) / TX;
    const long per_plane = (long)*tiles_h * *tiles_w;
    if (planes > 0x7fffffffL / per_plane) return false;
    *blocks = planes * per_plane;
    return true;
}

}  // namespace faoctasr
