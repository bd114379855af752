// Implicit-GEMM convolution for NARROW maps (an output phase narrower than SP_MIN_W = 24 pixels: the discriminators' 16x16 ... 3x3
// layers) on the f16 matrix cores with f16x2 split operands (split16.h): conv forward, conv input gradient, transposed-conv forward /
// input gradient, precision 3 only.  The exact-f32 narrow kernel (igemm_nm.hip) runs these layers on the f32 MFMA, 1/16 of the f16 rate;
// the wide split kernel (igemm_bf16x3.hip) cannot take them (its tiles are 32-pixel rows).
//
//   Y[M][pixels] = Wp[K][M]^T . im2col(X)[K][pixels],  K walked in k-steps of (16 channels, 1 tap), NX_KS k-steps per chunk.
//   * A = the f16x2 split weight image of the wide kernel (split_pack_kernel<true>, w * s(w) as hi / lo planes, the weights' absmax
//     slots in its tail): for one phase it is the run of k-steps (g16 * T + t) x [h][Mpad][8 ch], so a chunk of a 128-row block is 16
//     runs of 2 KiB, copied to LDS verbatim (8 dwordx4 loads + 8 ds_write_b128 per thread), one ds_read_b128 per fragment;
//   * B is gathered as in igemm_nm.hip: a thread keeps its pixel for the whole K loop; per chunk it computes ONE offset (its k-step's
//     tap) and issues 16 buffer loads whose channel planes are the scalar offsets.  The 16 values are scaled by s(x) and split into
//     hi / lo pairs (split_pair_scaled) and stored channel-innermost: [plane][k-step][h][pixel][8 ch], one ds_read_b128 per fragment;
//   * three v_mfma_f32_32x32x16_f16 per tile and k-step (lo*hi, hi*lo, hi*hi); both operands register-prefetched one chunk ahead;
//   * the accumulators are descaled with the two inverse scales one after the other (their product goes subnormal for small tensors);
//   * split-K WITHOUT atomics: small grids write descaled fp32 partials to a caller-owned workspace (faoctasr_conv_set_workspace) and
//     nx2_reduce_kernel sums them in slice order, then adds bias, applies the activation and adds the residual: two calls give
//     bit-identical outputs.  Without a workspace (or with FAOCTASR_CONV_NO_SPLIT_K) the grid is not split.
#include <type_traits>

#include "common.h"
#include "igemm_geom.h"
#include "split16.h"

namespace faoctasr {

typedef float f32x16x __attribute__((ext_vector_type(16)));
typedef unsigned u32x4x __attribute__((ext_vector_type(4)));

constexpr int NX_MT = 128, NX_NT = 64, NX_KS = 4;        // output rows, pixels per block; k-steps per chunk (one per wave's B share)

__global__ __launch_bounds__(256) void igemm_nm_x2_kernel(const float* __restrict__ x, const u32x4x* __restrict__ wp, const float* __restrict__ bias,
                                                          float* __restrict__ y, float* __restrict__ part, const SplitGeom g, const int ksplit,
                                                          const unsigned* __restrict__ x_slot, const unsigned* __restrict__ w_slot,
                                                          const float* __restrict__ res) {
    __shared__ u32x4x A_s[2 * NX_KS * 2 * NX_MT];        // [plane][k-step][h][m]      32 KiB
    __shared__ u32x4x B_s[2 * NX_KS * 2 * NX_NT];        // [plane][k-step][h][pixel]  16 KiB
    __shared__ int taps_s[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) taps_s[tid] = g.taps[tid];
    __syncthreads();
    const int l31 = lane & 31, lh = lane >> 5;
    const int ph = blockIdx.z / ksplit, ks = blockIdx.z - ph * ksplit;
    const int GH = g.gh[ph], GW = g.gw[ph];
    const long npix = (long)g.N * GH * GW;
    const long j0 = (long)blockIdx.x * NX_NT;
    if (j0 >= npix) return;
    const int m0 = blockIdx.y * NX_MT;
    const int t0 = g.t0[ph], T = g.t0[ph + 1] - t0;
    const int nchunks = (g.C >> 4) * T / NX_KS;          // C % 16 == 0 and (C / 16) T % NX_KS == 0: checked by the launcher
    const int cps = (nchunks + ksplit - 1) / ksplit;
    int ch0 = ks * cps, ch1 = ch0 + cps;
    ch0 = ch0 < nchunks ? ch0 : nchunks;
    ch1 = ch1 < nchunks ? ch1 : nchunks;                 // an empty slice (a phase with fewer chunks) still writes its zero partial
    const long chw = (long)g.IH * g.IW;

    // ---- B: this thread's pixel and k-step rg of every chunk
    const int jj = tid & 63, rg = tid >> 6;
    const long j = j0 + jj;
    const bool jv = j < npix;
    int a = 0, b = 0;
    unsigned img = 0;
    if (jv) {
        const int n = (int)(j / ((long)GH * GW));
        const int r = (int)(j - (long)n * GH * GW);
        a = r / GW;
        b = r - a * GW;
        img = 4u * (unsigned)((long)n * g.C * chw);      // N C IH IW < 2^29 checked by the launcher
    }
    const long x_bytes = (long)g.N * g.C * chw * 4;
    const auto xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)(x_bytes < 0x7ffffff0L ? x_bytes : 0x7ffffff0L), 0x00020000);
    const unsigned cstep = 4u * (unsigned)chw;
    const float sx = f16x2_scale(absmax_read(x_slot));
    // ---- A: piece p = tid + 256 i of a chunk's 2 planes x NX_KS k-steps x 2 halves x 128 rows; LDS slot p, image row (plane, k-step, h)
    const long plane4 = g.plane_stride >> 3, ph4 = g.pack_off[ph] >> 3;       // in 16-byte units (both multiples of 8 elements)
    const long row4 = g.Mpad;                                                  // one (k-step, h) row: Mpad x 8 elements

    u32x4x ra[8];
    float rb[16];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int p = tid + 256 * i, m = m0 + (p & 127), rw = (p >> 7) & 7, pl = p >> 10;
            ra[i] = m < g.Mpad ? wp[pl * plane4 + ph4 + ((long)ch * (2 * NX_KS) + rw) * row4 + m] : u32x4x{0u, 0u, 0u, 0u};
        }
        const int s = ch * NX_KS + rg, g16 = s / T, t = s - g16 * T;
        const int tp = taps_s[t0 + t];
        int iy = a * g.SI + (tp & 0xff) + g.oy0[ph], ix = b * g.SI + ((tp >> 8) & 0xff) + g.ox0[ph];
        if (g.reflect) {
            iy = iy < 0 ? -iy : iy; iy = iy >= g.IH ? 2 * g.IH - 2 - iy : iy;
            ix = ix < 0 ? -ix : ix; ix = ix >= g.IW ? 2 * g.IW - 2 - ix : ix;
        }
        const bool ok = jv && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
        const unsigned off = ok ? img + 4u * (unsigned)((long)g16 * 16 * chw + (long)iy * g.IW + ix) : 0x80000000u;
#pragma unroll
        for (int i = 0; i < 16; ++i) rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xsrd, off, (int)(i * cstep), 0));
    };

    // 4 waves = 2 (rows) x 2 (pixels): wave tile 64 rows x 32 pixels
    const int wm = wave >> 1, wn = wave & 1;
    f32x16x acc[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

    if (ch0 < ch1) load_chunk(ch0);
    for (int ch = ch0; ch < ch1; ++ch) {
        if (ch != ch0) __syncthreads();                  // the previous chunk's fragment reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) A_s[tid + 256 * i] = ra[i];
        {
            unsigned hi[8], lo[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) split_pair_scaled<true>(rb[2 * i], rb[2 * i + 1], sx, hi[i], lo[i]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                B_s[((0 * NX_KS + rg) * 2 + h) * NX_NT + jj] = u32x4x{hi[4 * h], hi[4 * h + 1], hi[4 * h + 2], hi[4 * h + 3]};
                B_s[((1 * NX_KS + rg) * 2 + h) * NX_NT + jj] = u32x4x{lo[4 * h], lo[4 * h + 1], lo[4 * h + 2], lo[4 * h + 3]};
            }
        }
        __syncthreads();
        if (ch + 1 < ch1) load_chunk(ch + 1);            // in flight under the MFMAs below
#pragma unroll
        for (int st = 0; st < NX_KS; ++st) {
            u32x4x ah[2], al[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int m = wm * 64 + mi * 32 + l31;
                ah[mi] = A_s[((0 * NX_KS + st) * 2 + lh) * NX_MT + m];
                al[mi] = A_s[((1 * NX_KS + st) * 2 + lh) * NX_MT + m];
            }
            const u32x4x bh = B_s[((0 * NX_KS + st) * 2 + lh) * NX_NT + wn * 32 + l31];
            const u32x4x bl = B_s[((1 * NX_KS + st) * 2 + lh) * NX_NT + wn * 32 + l31];
            // terms outermost: consecutive MFMAs go to different accumulators; the small terms first
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) mfma16<true>(al[mi], bh, acc[mi]);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) mfma16<true>(ah[mi], bl, acc[mi]);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) mfma16<true>(ah[mi], bh, acc[mi]);
        }
    }

    // ---- epilogue: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long jo = j0 + wn * 32 + l31;
    if (jo >= npix) return;
    const int no = (int)(jo / ((long)GH * GW));
    const int r0 = (int)(jo - (long)no * GH * GW);
    const int ao = r0 / GW, bo = r0 - ao * GW;
    const long ohw = (long)g.OH * g.OW;
    const long obase = (long)no * g.M * ohw + (long)(ao * g.SO + g.py[ph]) * g.OW + (bo * g.SO + g.px[ph]);
    const float inv_x = f16x2_inv_scale(absmax_read(x_slot)), inv_w = f16x2_inv_scale(split_w_absmax(w_slot));
    float* const dst = ksplit > 1 ? part + (long)ks * g.N * g.M * ohw : y;
    const bool fin = ksplit == 1;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int m = m0 + wm * 64 + mi * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (m < g.M) {
                const long o = obase + (long)m * ohw;
                float v = acc[mi][rr] * inv_x * inv_w;
                if (fin) {
                    if (bias) v += bias[m];
                    v = act_apply(v, g.act, g.slope);
                    if (res) v += res[o];
                }
                dst[o] = v;
            }
        }
}

// y = act(sum_ks part[ks] + bias) + res, the slices summed in order
__global__ __launch_bounds__(256) void nx2_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                                         const float* __restrict__ res, const long total, const int ksplit, const int M,
                                                         const long ohw, const int act, const float slope) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        float v = part[e];
        for (int k = 1; k < ksplit; ++k) v += part[(long)k * total + e];
        if (bias) v += bias[(e / ohw) % M];
        v = act_apply(v, act, slope);
        if (res) v += res[e];
        y[e] = v;
    }
}

// the grid and split of a layer this kernel takes; 0 when it does not take it
static int nx2_plan(const SplitGeom& g, long& gx, int& gy, int& ksplit, bool split_ok) {
    if (!g.f16 || g.M < 64 || (g.C & 15) || (long)g.N * g.C * g.IH * g.IW >= (1L << 29) || (long)g.N * g.M * g.OH * g.OW >= (1L << 30)) return 0;
    long maxpix = 0;
    int minchunks = 1 << 30;
    for (int p = 0; p < g.nphase; ++p) {
        const int T = g.t0[p + 1] - g.t0[p];
        if (T <= 0 || ((g.C >> 4) * T) % NX_KS) return 0;
        const long np = (long)g.N * g.gh[p] * g.gw[p];
        maxpix = np > maxpix ? np : maxpix;
        const int nc = (g.C >> 4) * T / NX_KS;
        minchunks = nc < minchunks ? nc : minchunks;
    }
    if (maxpix == 0) return 0;
    gx = (maxpix + NX_NT - 1) / NX_NT;
    gy = (g.M + NX_MT - 1) / NX_MT;
    const long blocks = gx * gy * g.nphase;
    // split K until ~2 blocks per CU exist, each slice still >= 8 chunks; every slice adds one write and one read of the output in fp32
    ksplit = 1;
    if (split_ok && blocks < 384) {
        ksplit = (int)((512 + blocks - 1) / blocks);
        if (ksplit > 8) ksplit = 8;
        if (ksplit > minchunks / 8) ksplit = minchunks / 8;
        if (ksplit < 1) ksplit = 1;
    }
    return 1;
}

long narrow_x2_workspace_floats(const SplitGeom& g) {
    long gx;
    int gy, ksplit;
    if (!nx2_plan(g, gx, gy, ksplit, true) || ksplit == 1) return 0;
    return (long)ksplit * g.N * g.M * g.OH * g.OW;
}

int narrow_x2_eligible(const SplitGeom& g) {
    long gx;
    int gy, ksplit;
    return nx2_plan(g, gx, gy, ksplit, false);
}

// 1 launched, 0 not eligible, <0 error.  `wp`: the f16x2 split image of this geometry (launch_split_pack); ws / ws_floats: the split-K
// workspace (may be null: then one slice)
int launch_narrow_x2(const float* x, const float* wp, const float* bias, float* y, SplitGeom& g, int act, float slope, hipStream_t s,
                     const unsigned* x_slot, const float* res, float* ws, long ws_floats) {
    g.act = act; g.slope = slope;
    long gx;
    int gy, ksplit;
    if (!nx2_plan(g, gx, gy, ksplit, !g_no_split_k && ws != nullptr)) return 0;
    const long total = (long)g.N * g.M * g.OH * g.OW;
    if (ksplit > 1 && ws_floats < (long)ksplit * total) ksplit = 1;
    const unsigned* w_slot = reinterpret_cast<const unsigned*>(wp) + split_scale_slot(g);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(g.nphase * ksplit));
    hipLaunchKernelGGL(igemm_nm_x2_kernel, grid, dim3(256), 0, s, x, reinterpret_cast<const u32x4x*>(wp), bias, y, ws, g, ksplit, x_slot, w_slot, res);
    int rc = check_launch("igemm_nm_x2");
    if (rc != FAOCTASR_OK || ksplit == 1) return rc == FAOCTASR_OK ? 1 : rc;
    long nb = (total + 255) / 256;
    nb = nb < 1024 ? nb : 1024;
    hipLaunchKernelGGL(nx2_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, s, ws, bias, y, res, total, ksplit, g.M, (long)g.OH * g.OW, act, slope);
    rc = check_launch("igemm_nm_x2 reduce");
    return rc == FAOCTASR_OK ? 1 : rc;
}

}  // namespace faoctasr
