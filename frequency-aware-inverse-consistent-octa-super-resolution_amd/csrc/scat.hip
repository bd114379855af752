// DTCWT scattering layers, fp32 (pytorch_wavelets scatternet/lowlevel.py ScatLayerj1_f, ScatLayerj2_f): a dual-tree level, the
// smoothed complex magnitude of its six orientations and the 2x2 average of its lowpass, in one launch; the backward likewise.
//
// The four kernels are the four of dtcwt.hip -- same tiles, LDS staging and index maps (dtcwt_dev.h) -- with the pointwise part of
// the layer in the place of their bandpass stores and loads:
//
// forward, in the registers that hold a quad's ll, lh, hl, hh after the second pass:
//   z_o = q2c of the quad (six complex values),  r_o = sqrt(re^2 + im^2 + b^2),  mag_o = r_o - b,  phase_o = (re / r_o, im / r_o)
//   low = mean of the quad's four ll values (pool) or ll itself at full resolution (level 1 only: the first stage of ScatLayerj2)
//   colour form (C == 3): r_o = sqrt(sum_c (re_c^2 + im_c^2) + b^2), one magnitude per orientation, phase_{o,c} = z_{o,c} / r_o; the
//   block runs its tile's three channels one after the other and keeps their 3 x 12 band values in registers.
//   phase == NULL: nothing is saved (a forward that no backward follows).
// backward, while staging a coefficient position (sr, sc) of the inverse:
//   ll = 0.25 dlow[sr / 2][sc / 2] (pool: the adjoint of the mean) or dlow[sr][sc];   z_o = dmag_o[sr / 2][sc / 2] phase_o[sr / 2][sc / 2],
//   c2q applied to the pairs; the two filter passes are the inverse's, on the analysis taps (level 1) or on them with trees a and
//   b swapped (level 2) -- the exact adjoint.  The colour form is a zero channel stride of dmag.
//
// Three-filter ("_bp") banks, ScatLayerj1_rot_f / ScatLayerj2_rot_f: every kernel has the compile-time form BP of its dtcwt.hip twin --
// forward  ba = row(x, h2), hh = col(ba, h2);  backward  hi = col(hl, h0), ba = col(hh, h2), dx = (row(hi, h1) + row(lo, h0)) + row(ba, h2)
// -- and the pointwise part is untouched.  The two-filter forms compile to the instructions they had before.
//
// Addressing, in elements, rows always contiguous: low (n, c) strides, mag / dmag (n, orientation, c) strides, so a launch writes
// into (reads from) slices of the layer's output Z (its cotangent); phase is a contiguous (N, 6, C, H', W', 2) tensor, one float2
// per value.  The input x takes (n, c, row) strides; dx is contiguous.  Taps travel by value, nothing is allocated, no state,
// every sum in a fixed order: capturable and bit-reproducible.
#include "dtcwt_dev.h"

namespace faoctasr {

struct ScLow { long n, c; };
struct ScMag { long n, o, c; };

// magnitudes and phasors of one orientation over NC channels (NC == 1, or 3 reduced to one magnitude)
template <int NC>
__device__ __forceinline__ void sc_emit(const float2 (&z)[NC], float* mag, long mag_c, float2* ph, long ph_c, float b, float b2, bool colour) {
    if (colour) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) s += z[k].x * z[k].x + z[k].y * z[k].y;
        const float r = sqrtf(s + b2);
        *mag = r - b;
        if (ph) {
#pragma unroll
            for (int k = 0; k < NC; ++k) ph[k * ph_c] = make_float2(z[k].x / r, z[k].y / r);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const float r = sqrtf(z[k].x * z[k].x + z[k].y * z[k].y + b2);
            mag[k * mag_c] = r - b;
            if (ph) ph[k * ph_c] = make_float2(z[k].x / r, z[k].y / r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 forward: x [H, W] even -> low [H/2, W/2] (pool) or [H, W], mag and phase [H/2, W/2].  COLOUR: a block takes the three
// channels of its tile (the grid has N planes), else one (N * C planes)
// ---------------------------------------------------------------------------------------------------------------------------
template <bool COLOUR, bool BP>
__global__ __launch_bounds__(256) void scat_fwd_j1(const float* __restrict__ x, DtLow xs, float* __restrict__ low, ScLow ls, int pool,
                                                   float* __restrict__ mag, ScMag ms, float2* __restrict__ phase, float b, float b2, int C, int H,
                                                   int W, int tiles_h, int tiles_w, int L0, int L1, int sym, typename DtBank<BP>::T1 taps) {
    constexpr int NC = COLOUR ? 3 : 1;
    __shared__ float patch[J1_PR][J1_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[J1_PR][J1_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? J1_PR : 1][J1_TW];
    const int tid = threadIdx.x;
    int bi = blockIdx.x;
    const int tw = bi % tiles_w; bi /= tiles_w;
    const int th = bi % tiles_h;
    const long plane = bi / tiles_h;
    const long n = COLOUR ? plane : plane / C, c0 = COLOUR ? 0 : plane % C;
    const int oi0 = th * J1_TH, oj0 = tw * J1_TW;
    const int hm = dt_halo1<BP>(L0, L1, taps), a0 = hm - (L0 >> 1), a1 = hm - (L1 >> 1);
    const int rows = J1_TH + 2 * hm, cols = J1_TW + 2 * hm;               // <= J1_PR, J1_PC
    const int qi = tid >> 5, qj = tid & 31;                               // H pass: a thread owns one 2x2 quad of the tile
    const int oi = oi0 + 2 * qi, oj = oj0 + 2 * qj;
    const bool live = oi < H && oj < W;                                   // H, W even: a quad is inside or outside as a whole
    const int OH = H >> 1, OW = W >> 1, pi = oi >> 1, pj = oj >> 1;
    float2 z[6][NC];

#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const long c = c0 + k;
        const float* xp = x + n * xs.n + c * xs.c;
        for (int r = tid >> 6; r < rows; r += 4) {
            const int sr = dt_map(oi0 - hm + r, H, sym);
            for (int cc = tid & 63; cc < cols; cc += 64) {
                const int sc = dt_map(oj0 - hm + cc, W, sym);
                patch[r][cc] = (sr >= 0 && sc >= 0) ? xp[sr * xs.r + sc] : 0.f;
            }
        }
        __syncthreads();

        {   // W pass: thread (r, cc) filters patch row r at tile column cc
            const int cc = tid & 63;
            for (int r = tid >> 6; r < rows; r += 4) {
                float lo = 0.f, hv = 0.f;
                for (int t = 0; t < L0; ++t) lo = fmaf(taps.f0[t], patch[r][cc + t + a0], lo);
                for (int t = 0; t < L1; ++t) hv = fmaf(taps.f1[t], patch[r][cc + t + a1], hv);
                mid_lo[r][cc] = lo;
                mid_hi[r][cc] = hv;
                if constexpr (BP) {
                    const int a2 = hm - (taps.L2 >> 1);
                    float bv = 0.f;
                    for (int t = 0; t < taps.L2; ++t) bv = fmaf(taps.f2[t], patch[r][cc + t + a2], bv);
                    mid_ba[r][cc] = bv;
                }
            }
        }
        __syncthreads();                                                  // the next channel's W pass follows its own barrier

        if (live) {
            float2 vll[2], vlh[2], vhl[2], vhh[2];
            for (int d = 0; d < 2; ++d) {
                float2 s = make_float2(0.f, 0.f), u = s, p = s, q = s;
                for (int t = 0; t < L0; ++t) {
                    const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + a0][2 * qj]);
                    const float2 w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + a0][2 * qj]);
                    s.x = fmaf(taps.f0[t], v.x, s.x); s.y = fmaf(taps.f0[t], v.y, s.y);
                    p.x = fmaf(taps.f0[t], w.x, p.x); p.y = fmaf(taps.f0[t], w.y, p.y);
                }
                for (int t = 0; t < L1; ++t) {
                    const float2 v = *reinterpret_cast<const float2*>(&mid_lo[2 * qi + d + t + a1][2 * qj]);
                    float2 w;
                    if constexpr (!BP) w = *reinterpret_cast<const float2*>(&mid_hi[2 * qi + d + t + a1][2 * qj]);
                    u.x = fmaf(taps.f1[t], v.x, u.x); u.y = fmaf(taps.f1[t], v.y, u.y);
                    if constexpr (!BP) { q.x = fmaf(taps.f1[t], w.x, q.x); q.y = fmaf(taps.f1[t], w.y, q.y); }
                }
                if constexpr (BP) {                                       // hh = col(ba, h2)
                    const int a2 = hm - (taps.L2 >> 1);
                    for (int t = 0; t < taps.L2; ++t) {
                        const float2 w = *reinterpret_cast<const float2*>(&mid_ba[2 * qi + d + t + a2][2 * qj]);
                        q.x = fmaf(taps.f2[t], w.x, q.x); q.y = fmaf(taps.f2[t], w.y, q.y);
                    }
                }
                vll[d] = s; vlh[d] = u; vhl[d] = p; vhh[d] = q;
            }
            float* lp = low + n * ls.n + c * ls.c;
            if (pool) {
                lp[(long)pi * OW + pj] = 0.25f * ((vll[0].x + vll[0].y) + (vll[1].x + vll[1].y));
            } else {
                *reinterpret_cast<float2*>(lp + (long)oi * W + oj) = vll[0];
                *reinterpret_cast<float2*>(lp + (long)(oi + 1) * W + oj) = vll[1];
            }
            dt_q2c_val(vlh[0], vlh[1], &z[0][k], &z[5][k]);
            dt_q2c_val(vhh[0], vhh[1], &z[1][k], &z[4][k]);
            dt_q2c_val(vhl[0], vhl[1], &z[2][k], &z[3][k]);
        }
    }
    if (!live) return;
    const long hw = (long)OH * OW, at = (long)pi * OW + pj;
#pragma unroll
    for (int o = 0; o < 6; ++o)
        sc_emit<NC>(z[o], mag + n * ms.n + o * ms.o + c0 * ms.c + at, ms.c, phase ? phase + ((n * 6 + o) * C + c0) * hw + at : nullptr, hw, b, b2,
                    COLOUR);
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 2 forward: x [H, W] (multiples of 4) -> low [H/4, W/4] (the 2x2 mean of the level's lowpass), mag and phase [H/4, W/4]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool COLOUR, bool BP>
__global__ __launch_bounds__(256) void scat_fwd_j2(const float* __restrict__ x, DtLow xs, float* __restrict__ low, ScLow ls,
                                                   float* __restrict__ mag, ScMag ms, float2* __restrict__ phase, float b, float b2, int C, int H,
                                                   int W, int tiles_h, int tiles_w, int m, typename DtBank<BP>::T2 taps) {
    constexpr int NC = COLOUR ? 3 : 1;
    __shared__ __attribute__((aligned(16))) float patch[F2_PR][F2_PC];
    __shared__ __attribute__((aligned(16))) float mid_lo[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_hi[F2_PR][F2_TW];
    __shared__ __attribute__((aligned(16))) float mid_ba[BP ? F2_PR : 1][F2_TW];
    const int tid = threadIdx.x;
    int bi = blockIdx.x;
    const int tw = bi % tiles_w; bi /= tiles_w;
    const int th = bi % tiles_h;
    const long plane = bi / tiles_h;
    if (COLOUR) C = 3;
    const long n = COLOUR ? plane : plane / C, c0 = COLOUR ? 0 : plane % C;
    const int OH = H >> 2, OW = W >> 2;                                    // of low, mag and phase
    const int i0 = th * (F2_TH / 2), j0 = tw * (F2_TW / 2);               // first quad row / column = first index of the trees
    const int rows = 2 * F2_TH + 2 * m - 4, cols = 2 * F2_TW + 2 * m - 4;  // <= F2_PR, F2_PC; patch (r, cc) is x position 4 i0 + 2 - m + r
    // H pass: 4 x 32 quads; threads 0..127 take the W-lowpass plane (ll, lh), threads 128..255 the W-highpass plane (hl, hh)
    const int path = tid >> 7, qi = (tid & 127) >> 5, qj = tid & 31;
    const int pi = i0 + qi, pj = j0 + qj;
    const bool live = pi < OH && pj < OW;
    float2 za[4][NC];                                                     // path 0: lh z1, z2 (15, 165); path 1: hl z1, z2 (75, 105), hh z1, z2 (45, 135)

#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const long c = c0 + k;
        const float* xp = x + n * xs.n + c * xs.c;
        for (int r = tid >> 6; r < rows; r += 4) {
            const int sr = dt_map(4 * i0 + 2 - m + r, H, 1);
            for (int cc = tid & 63; cc < cols; cc += 64)
                patch[r][cc] = xp[sr * xs.r + dt_map(4 * j0 + 2 - m + cc, W, 1)];
        }
        __syncthreads();

        {   // W pass: tile column cc = 2 i + p; the float2 at patch column 4 i + 2 t holds the samples at offsets 2 - m and 3 - m
            const int cc = tid & 63, i = cc >> 1, p = cc & 1;
            for (int r = tid >> 6; r < rows; r += 4) {
                float lo = 0.f, hv = 0.f, bv = 0.f;
                for (int t = 0; t < m; ++t) {
                    const float2 v = *reinterpret_cast<const float2*>(&patch[r][4 * i + 2 * t]);
                    lo = fmaf(p ? taps.lo1[t] : taps.lo0[t], p ? v.y : v.x, lo);
                    hv = fmaf(p ? taps.hi1[t] : taps.hi0[t], p ? v.x : v.y, hv);
                    if constexpr (BP) bv = fmaf(p ? taps.ba1[t] : taps.ba0[t], p ? v.x : v.y, bv);
                }
                mid_lo[r][cc] = lo;
                mid_hi[r][cc] = hv;
                if constexpr (BP) mid_ba[r][cc] = bv;
            }
        }
        __syncthreads();

        if (live) {
            float2 l0 = make_float2(0.f, 0.f), l1 = l0, h0 = l0, h1 = l0;     // lowpass call rows 2qi, 2qi+1; highpass call likewise
            for (int t = 0; t < m; ++t) {
                const float* mp = path ? &mid_hi[4 * qi + 2 * t][2 * qj] : &mid_lo[4 * qi + 2 * t][2 * qj];
                const float2 r0 = *reinterpret_cast<const float2*>(mp), r1 = *reinterpret_cast<const float2*>(mp + F2_TW);
                l0.x = fmaf(taps.lo0[t], r0.x, l0.x); l0.y = fmaf(taps.lo0[t], r0.y, l0.y);
                l1.x = fmaf(taps.lo1[t], r1.x, l1.x); l1.y = fmaf(taps.lo1[t], r1.y, l1.y);
                if constexpr (BP) {                                       // path 1: hh from the W-bandpass plane on the bandpass taps
                    const float* bp = path ? &mid_ba[4 * qi + 2 * t][2 * qj] : mp;
                    const float2 b0 = *reinterpret_cast<const float2*>(bp), b1 = *reinterpret_cast<const float2*>(bp + F2_TW);
                    const float k0 = path ? taps.ba0[t] : taps.hi0[t], k1 = path ? taps.ba1[t] : taps.hi1[t];
                    h0.x = fmaf(k0, b1.x, h0.x); h0.y = fmaf(k0, b1.y, h0.y);
                    h1.x = fmaf(k1, b0.x, h1.x); h1.y = fmaf(k1, b0.y, h1.y);
                } else {
                    h0.x = fmaf(taps.hi0[t], r1.x, h0.x); h0.y = fmaf(taps.hi0[t], r1.y, h0.y);
                    h1.x = fmaf(taps.hi1[t], r0.x, h1.x); h1.y = fmaf(taps.hi1[t], r0.y, h1.y);
                }
            }
            if (path) {
                dt_q2c_val(l0, l1, &za[0][k], &za[1][k]);                 // hl
                dt_q2c_val(h0, h1, &za[2][k], &za[3][k]);                 // hh
            } else {
                low[n * ls.n + c * ls.c + (long)pi * OW + pj] = 0.25f * ((l0.x + l0.y) + (l1.x + l1.y));
                dt_q2c_val(h0, h1, &za[0][k], &za[1][k]);                 // lh
                za[2][k] = za[3][k] = make_float2(0.f, 0.f);
            }
        }
    }
    if (!live) return;
    const long hw = (long)OH * OW, at = (long)pi * OW + pj;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!path && j >= 2) break;
        const int o = path ? (j == 0 ? 2 : j == 1 ? 3 : j == 2 ? 1 : 4) : (j == 0 ? 0 : 5);
        sc_emit<NC>(za[j], mag + n * ms.n + o * ms.o + c0 * ms.c + at, ms.c, phase ? phase + ((n * 6 + o) * C + c0) * hw + at : nullptr, hw, b, b2,
                    COLOUR);
    }
}

// one coefficient position (sr, sc) of the four full-resolution planes ll, lh, hl, hh from the layer's cotangents and phasors
__device__ __forceinline__ void sc_stage(const float* lp, int pool, int lw, const float* dm, long mo, const float2* ph, long po, int pw, int sr,
                                         int sc, float* o0, float* o1, float* o2, float* o3) {
    *o0 = pool ? 0.25f * lp[(long)(sr >> 1) * lw + (sc >> 1)] : lp[(long)sr * lw + sc];
    const long at = (long)(sr >> 1) * pw + (sc >> 1);
    const int pr = sr & 1, pc = sc & 1;
    const bool im = pr ^ pc;                                              // (0,1) and (1,0) take the imaginary parts
    float w[6];
#pragma unroll
    for (int o = 0; o < 6; ++o) {
        const float2 p = ph[o * po + at];
        w[o] = dm[o * mo + at] * (im ? p.y : p.x);
    }
    *o1 = dt_c2q_val(w[0], w[5], pr, pc);                                 // lh: 15, 165
    *o2 = dt_c2q_val(w[2], w[3], pr, pc);                                 // hl: 75, 105
    *o3 = dt_c2q_val(w[1], w[4], pr, pc);                                 // hh: 45, 135
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 1 backward: dlow [H/2, W/2] (pool) or [H, W], dmag and phase [H/2, W/2] -> dx [H, W]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void scat_bwd_j1(const float* __restrict__ dlow, ScLow ls, int pool, const float* __restrict__ dmag, ScMag ms,
                                                   const float2* __restrict__ phase, float* __restrict__ dx, int C, int H, int W, int tiles_h,
                                                   int tiles_w, int L0, int L1, int sym, typename DtBank<BP>::T1 taps) {
    __shared__ float cf[4][J1_PR][J1_PC];
    __shared__ float mid_lo[J1_TH][J1_PC], mid_hi[J1_TH][J1_PC], mid_ba[BP ? J1_TH : 1][J1_PC];
    const int tid = threadIdx.x;
    int bi = blockIdx.x;
    const int tw = bi % tiles_w; bi /= tiles_w;
    const int th = bi % tiles_h;
    const long plane = bi / tiles_h;
    const long n = plane / C, c = plane % C;
    const int t0 = th * J1_TH, s0 = tw * J1_TW;
    const int hm = dt_halo1<BP>(L0, L1, taps), a0 = hm - (L0 >> 1), a1 = hm - (L1 >> 1);
    const int rows = J1_TH + 2 * hm, cols = J1_TW + 2 * hm;
    const int OW = W >> 1;
    const long hw = (long)(H >> 1) * OW;
    const float* lp = dlow + n * ls.n + c * ls.c;
    const float* dm = dmag + n * ms.n + c * ms.c;
    const float2* ph = phase + (n * 6 * C + c) * hw;

    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(t0 - hm + r, H, sym);
        for (int cc = tid & 63; cc < cols; cc += 64) {
            const int sc = dt_map(s0 - hm + cc, W, sym);
            if (sr >= 0 && sc >= 0) sc_stage(lp, pool, pool ? OW : W, dm, ms.o, ph, C * hw, OW, sr, sc, &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
            else cf[0][r][cc] = cf[1][r][cc] = cf[2][r][cc] = cf[3][r][cc] = 0.f;
        }
    }
    __syncthreads();

    // H pass: lo = col(lh, g1) + col(ll, g0), hi = col(hh, g1) + col(hl, g0), for every tile row and patch column
    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {
        for (int cc = tid & 63; cc < cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            for (int t = 0; t < L1; ++t) {
                l1 = fmaf(taps.f1[t], cf[1][tt + t + a1][cc], l1);
                if constexpr (!BP) h1 = fmaf(taps.f1[t], cf[3][tt + t + a1][cc], h1);
            }
            for (int t = 0; t < L0; ++t) {
                h0 = fmaf(taps.f0[t], cf[2][tt + t + a0][cc], h0);
                l0 = fmaf(taps.f0[t], cf[0][tt + t + a0][cc], l0);
            }
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) {                                           // hi = col(hl, h0), ba = col(hh, h2)
                const int a2 = hm - (taps.L2 >> 1);
                for (int t = 0; t < taps.L2; ++t) h1 = fmaf(taps.f2[t], cf[3][tt + t + a2][cc], h1);
                mid_hi[tt][cc] = h0;
                mid_ba[tt][cc] = h1;
            } else {
                mid_hi[tt][cc] = h1 + h0;
            }
        }
    }
    __syncthreads();

    float* yp = dx + plane * H * (long)W;
    const int ss = tid & 63, s = s0 + ss;
    for (int tt = tid >> 6; tt < J1_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= H || s >= W) continue;
        float vh = 0.f, vl = 0.f;
        for (int k = 0; k < L1; ++k) vh = fmaf(taps.f1[k], mid_hi[tt][ss + k + a1], vh);
        for (int k = 0; k < L0; ++k) vl = fmaf(taps.f0[k], mid_lo[tt][ss + k + a0], vl);
        if constexpr (BP) {
            const int a2 = hm - (taps.L2 >> 1);
            float vb = 0.f;
            for (int k = 0; k < taps.L2; ++k) vb = fmaf(taps.f2[k], mid_ba[tt][ss + k + a2], vb);
            yp[(long)t * W + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * W + s] = vh + vl;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// level 2 backward: dlow, dmag and phase [R/2, Q/2] -> dx [2R, 2Q]; always symmetric
// ---------------------------------------------------------------------------------------------------------------------------
template <bool BP>
__global__ __launch_bounds__(256) void scat_bwd_j2(const float* __restrict__ dlow, ScLow ls, const float* __restrict__ dmag, ScMag ms,
                                                   const float2* __restrict__ phase, float* __restrict__ dx, int C, int R, int Q, int tiles_h,
                                                   int tiles_w, int m2, typename DtBank<BP>::TI taps) {
    __shared__ float cf[4][I2_PR][I2_PC];
    __shared__ float mid_lo[I2_TH][I2_PC], mid_hi[I2_TH][I2_PC], mid_ba[BP ? I2_TH : 1][I2_PC];
    __shared__ float tl[BP ? 3 : 2][4][DT_MAXL / 2];
    __shared__ int td[BP ? 3 : 2][4];
    const int tid = threadIdx.x;
    int bi = blockIdx.x;
    const int tw = bi % tiles_w; bi /= tiles_w;
    const int th = bi % tiles_h;
    const long plane = bi / tiles_h;
    const long n = plane / C, c = plane % C;
    const int t0 = th * I2_TH, s0 = tw * I2_TW, OH = 2 * R, OW = 2 * Q;
    const int i0 = t0 >> 2, j0 = s0 >> 2;
    const int rows = I2_TH / 2 + 2 * m2, cols = I2_TW / 2 + 2 * m2;      // patch (r, cc) is coefficient position 2 i0 - m2 + r
    const int PW = Q >> 1;
    const long hw = (long)(R >> 1) * PW;
    const float* lp = dlow + n * ls.n + c * ls.c;
    const float* dm = dmag + n * ms.n + c * ms.c;
    const float2* ph = phase + (n * 6 * C + c) * hw;

    if (tid < 4 * (DT_MAXL / 2)) {                                        // the per-phase taps, for the lane-varying phase of the W pass
        tl[0][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.lo[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
        tl[1][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.hi[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
        if constexpr (BP) tl[2][tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)] = taps.ba[tid / (DT_MAXL / 2)][tid % (DT_MAXL / 2)];
    }
    if (tid < 4) {
        td[0][tid] = taps.dlo[tid]; td[1][tid] = taps.dhi[tid];
        if constexpr (BP) td[2][tid] = taps.dba[tid];
    }
    for (int r = tid >> 6; r < rows; r += 4) {
        const int sr = dt_map(2 * i0 - m2 + r, R, 1);
        for (int cc = tid & 63; cc < cols; cc += 64)
            sc_stage(lp, 1, PW, dm, ms.o, ph, C * hw, PW, sr, dt_map(2 * j0 - m2 + cc, Q, 1), &cf[0][r][cc], &cf[1][r][cc], &cf[2][r][cc], &cf[3][r][cc]);
    }
    __syncthreads();

    // H pass: a wave takes a tile row (its phase q is uniform), lanes the patch columns
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int q = tt & 3, ii = tt >> 2;                               // t0 is a multiple of 4
        const int rl = 2 * ii + td[0][q], rh = 2 * ii + td[1][q], rb = 2 * ii + td[BP ? 2 : 1][q];
        for (int cc = tid & 63; cc < cols; cc += 64) {
            float l1 = 0.f, l0 = 0.f, h1 = 0.f, h0 = 0.f;
            for (int t = 0; t < m2; ++t) {
                l1 = fmaf(tl[1][q][t], cf[1][rh + 2 * t][cc], l1);
                h1 = fmaf(tl[BP ? 2 : 1][q][t], cf[3][rb + 2 * t][cc], h1);         // BP: ba = col(hh, h2)
                h0 = fmaf(tl[0][q][t], cf[2][rl + 2 * t][cc], h0);
                l0 = fmaf(tl[0][q][t], cf[0][rl + 2 * t][cc], l0);
            }
            mid_lo[tt][cc] = l1 + l0;
            if constexpr (BP) { mid_hi[tt][cc] = h0; mid_ba[tt][cc] = h1; }
            else mid_hi[tt][cc] = h1 + h0;
        }
    }
    __syncthreads();

    float* yp = dx + plane * OH * (long)OW;
    const int ss = tid & 63, s = s0 + ss, q = ss & 3, jj = ss >> 2;
    const int cl = 2 * jj + td[0][q], ch = 2 * jj + td[1][q];
    for (int tt = tid >> 6; tt < I2_TH; tt += 4) {
        const int t = t0 + tt;
        if (t >= OH || s >= OW) continue;
        float vh = 0.f, vl = 0.f;
        for (int k = 0; k < m2; ++k) vh = fmaf(tl[1][q][k], mid_hi[tt][ch + 2 * k], vh);
        for (int k = 0; k < m2; ++k) vl = fmaf(tl[0][q][k], mid_lo[tt][cl + 2 * k], vl);
        if constexpr (BP) {
            const int cb = 2 * jj + td[2][q];
            float vb = 0.f;
            for (int k = 0; k < m2; ++k) vb = fmaf(tl[2][q][k], mid_ba[tt][cb + 2 * k], vb);
            yp[(long)t * OW + s] = (vh + vl) + vb;
        } else {
            yp[(long)t * OW + s] = vh + vl;
        }
    }
}

static int sc_common(const char* what, const void* a, const void* b, const void* c, int colour, int C) {
    if (!a || !b || !c) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (colour && C != 3) return fail(FAOCTASR_EINVAL, "%s: the colour form takes 3 channels, got %d", what, C);
    return FAOCTASR_OK;
}

}  // namespace faoctasr

using namespace faoctasr;

// The entry points of a kernel's two forms share everything but the taps: run_* takes them checked and packed.
template <bool BP>
static int run_fwd_j1(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                      float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C,
                      int H, int W, int L0, int L1, const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    int rc;
    if ((rc = sc_common(what, x, low, mag, colour, C))) return rc;
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be even and at least 2", what, H, W);
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    const int tiles_h = (H + J1_TH - 1) / J1_TH, tiles_w = (W + J1_TW - 1) / J1_TW;
    long blocks;
    if ((rc = dt_blocks(what, N, colour ? 1 : C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const ScLow ls{low_sn, low_sc};
    const ScMag ms{mag_sn, mag_so, mag_sc};
    if (colour)
        hipLaunchKernelGGL((scat_fwd_j1<true, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, pool != 0, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    else
        hipLaunchKernelGGL((scat_fwd_j1<false, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, pool != 0, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, L0, L1, mode == 1, t);
    return check_launch(what);
}

template <bool BP>
static int run_fwd_j2(const char* what, const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                      long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C, int H, int W,
                      int m, const typename DtBank<BP>::T2& t, faoctasr_stream_t stream) {
    int rc;
    if ((rc = sc_common(what, x, low, mag, colour, C))) return rc;
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be multiples of 4", what, H, W);
    const int tiles_h = (H / 2 + F2_TH - 1) / F2_TH, tiles_w = (W / 2 + F2_TW - 1) / F2_TW;
    long blocks;
    if ((rc = dt_blocks(what, N, colour ? 1 : C, tiles_h, tiles_w, &blocks))) return rc;
    const DtLow xs{x_sn, x_sc, x_sr};
    const ScLow ls{low_sn, low_sc};
    const ScMag ms{mag_sn, mag_so, mag_sc};
    if (colour)
        hipLaunchKernelGGL((scat_fwd_j2<true, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, m, t);
    else
        hipLaunchKernelGGL((scat_fwd_j2<false, BP>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, xs, low, ls, mag, ms,
                           reinterpret_cast<float2*>(phase), bias, bias2, C, H, W, tiles_h, tiles_w, m, t);
    return check_launch(what);
}

template <bool BP>
static int run_bwd_j1(const char* what, const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                      long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, int L0, int L1,
                      const typename DtBank<BP>::T1& t, int mode, faoctasr_stream_t stream) {
    if (!dlow || !dmag || !phase || !dx) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(FAOCTASR_EINVAL, "%s: H %d W %d must be even and at least 2", what, H, W);
    if (mode < 0 || mode > 6) return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d", what, mode);
    const int tiles_h = (H + J1_TH - 1) / J1_TH, tiles_w = (W + J1_TW - 1) / J1_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(scat_bwd_j1<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dlow, ScLow{dlow_sn, dlow_sc}, pool != 0, dmag,
                       ScMag{dmag_sn, dmag_so, dmag_sc}, reinterpret_cast<const float2*>(phase), dx, C, H, W, tiles_h, tiles_w, L0, L1,
                       mode == 1, t);
    return check_launch(what);
}

template <bool BP>
static int run_bwd_j2(const char* what, const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so,
                      long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, int m, const typename DtBank<BP>::TI& t,
                      faoctasr_stream_t stream) {
    if (!dlow || !dmag || !phase || !dx) return fail(FAOCTASR_EINVAL, "%s: null pointer", what);
    if (H < 4 || W < 4 || (H & 3) || (W & 3)) return fail(FAOCTASR_EINVAL, "%s: the result's H %d W %d must be multiples of 4", what, H, W);
    const int tiles_h = (H + I2_TH - 1) / I2_TH, tiles_w = (W + I2_TW - 1) / I2_TW;
    long blocks;
    int rc;
    if ((rc = dt_blocks(what, N, C, tiles_h, tiles_w, &blocks))) return rc;
    hipLaunchKernelGGL(scat_bwd_j2<BP>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dlow, ScLow{dlow_sn, dlow_sc}, dmag,
                       ScMag{dmag_sn, dmag_so, dmag_sc}, reinterpret_cast<const float2*>(phase), dx, C, H / 2, W / 2, tiles_h, tiles_w, m / 2, t);
    return check_launch(what);
}

extern "C" int faoctasr_scat_fwd_j1(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                                    float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2,
                                    long N, int C, int H, int W, const float* h0, int L0, const float* h1, int L1, int mode,
                                    faoctasr_stream_t stream) {
    DtTaps1 t;
    const int rc = dt_taps1("scat_fwd_j1", h0, L0, h1, L1, &t);
    if (rc) return rc;
    return run_fwd_j1<false>("scat_fwd_j1", x, x_sn, x_sc, x_sr, low, low_sn, low_sc, pool, mag, mag_sn, mag_so, mag_sc, phase, colour, bias, bias2,
                             N, C, H, W, L0, L1, t, mode, stream);
}

extern "C" int faoctasr_scat_fwd_j1_bp(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, int pool,
                                       float* mag, long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2,
                                       long N, int C, int H, int W, const float* h0, int L0, const float* h1, int L1, const float* h2,
                                       int L2, int mode, faoctasr_stream_t stream) {
    DtTaps1R t;
    const int rc = dt_taps1r("scat_fwd_j1_bp", h0, L0, h1, L1, h2, L2, &t);
    if (rc) return rc;
    return run_fwd_j1<true>("scat_fwd_j1_bp", x, x_sn, x_sc, x_sr, low, low_sn, low_sc, pool, mag, mag_sn, mag_so, mag_sc, phase, colour, bias,
                            bias2, N, C, H, W, L0, L1, t, mode, stream);
}

extern "C" int faoctasr_scat_fwd_j2(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                                    long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N, int C,
                                    int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b, int m,
                                    faoctasr_stream_t stream) {
    const int rc = dt_taps2_check("scat_fwd_j2", h0a, h0b, h1a, h1b, m);
    if (rc) return rc;
    DtTaps2 t = {};
    dt_taps2_fill(&t, h0a, h0b, h1a, h1b, m);
    return run_fwd_j2<false>("scat_fwd_j2", x, x_sn, x_sc, x_sr, low, low_sn, low_sc, mag, mag_sn, mag_so, mag_sc, phase, colour, bias, bias2, N, C,
                             H, W, m, t, stream);
}

extern "C" int faoctasr_scat_fwd_j2_bp(const float* x, long x_sn, long x_sc, long x_sr, float* low, long low_sn, long low_sc, float* mag,
                                       long mag_sn, long mag_so, long mag_sc, float* phase, int colour, float bias, float bias2, long N,
                                       int C, int H, int W, const float* h0a, const float* h0b, const float* h1a, const float* h1b,
                                       const float* h2a, const float* h2b, int m, faoctasr_stream_t stream) {
    const int rc = dt_taps2r_check("scat_fwd_j2_bp", h0a, h0b, h1a, h1b, h2a, h2b, m);
    if (rc) return rc;
    DtTaps2R t = {};
    dt_taps2_fill(&t, h0a, h0b, h1a, h1b, h2a, h2b, m);
    return run_fwd_j2<true>("scat_fwd_j2_bp", x, x_sn, x_sc, x_sr, low, low_sn, low_sc, mag, mag_sn, mag_so, mag_sc, phase, colour, bias, bias2, N,
                            C, H, W, m, t, stream);
}

extern "C" int faoctasr_scat_bwd_j1(const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                                    long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, const float* h0, int L0,
                                    const float* h1, int L1, int mode, faoctasr_stream_t stream) {
    DtTaps1 t;
    const int rc = dt_taps1("scat_bwd_j1", h0, L0, h1, L1, &t);
    if (rc) return rc;
    return run_bwd_j1<false>("scat_bwd_j1", dlow, dlow_sn, dlow_sc, pool, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, L0, L1, t, mode,
                             stream);
}

extern "C" int faoctasr_scat_bwd_j1_bp(const float* dlow, long dlow_sn, long dlow_sc, int pool, const float* dmag, long dmag_sn, long dmag_so,
                                       long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, const float* h0, int L0,
                                       const float* h1, int L1, const float* h2, int L2, int mode, faoctasr_stream_t stream) {
    DtTaps1R t;
    const int rc = dt_taps1r("scat_bwd_j1_bp", h0, L0, h1, L1, h2, L2, &t);
    if (rc) return rc;
    return run_bwd_j1<true>("scat_bwd_j1_bp", dlow, dlow_sn, dlow_sc, pool, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, L0, L1, t, mode,
                            stream);
}

extern "C" int faoctasr_scat_bwd_j2(const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so, long dmag_sc,
                                    const float* phase, float* dx, long N, int C, int H, int W, const float* h0a, const float* h0b,
                                    const float* h1a, const float* h1b, int m, faoctasr_stream_t stream) {
    const int rc = dt_taps2_check("scat_bwd_j2", h0a, h0b, h1a, h1b, m);
    if (rc) return rc;
    DtTapsI t = {};
    dtcwt_ifilt_taps(h0a, h0b, m, 0, t.lo, t.dlo);                        // the inverse on g0a = h0b, g0b = h0a: colifilt(X, g0b, g0a, False)
    dtcwt_ifilt_taps(h1a, h1b, m, 1, t.hi, t.dhi);                        // g1a = h1b, g1b = h1a: colifilt(X, g1b, g1a, True)
    return run_bwd_j2<false>("scat_bwd_j2", dlow, dlow_sn, dlow_sc, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, m, t, stream);
}

extern "C" int faoctasr_scat_bwd_j2_bp(const float* dlow, long dlow_sn, long dlow_sc, const float* dmag, long dmag_sn, long dmag_so,
                                       long dmag_sc, const float* phase, float* dx, long N, int C, int H, int W, const float* h0a,
                                       const float* h0b, const float* h1a, const float* h1b, const float* h2a, const float* h2b, int m,
                                       faoctasr_stream_t stream) {
    const int rc = dt_taps2r_check("scat_bwd_j2_bp", h0a, h0b, h1a, h1b, h2a, h2b, m);
    if (rc) return rc;
    DtTapsIR t = {};
    dtcwt_ifilt_taps(h0a, h0b, m, 0, t.lo, t.dlo);                        // the inverse on g0a = h0b, g0b = h0a: colifilt(X, g0b, g0a, False)
    dtcwt_ifilt_taps(h1a, h1b, m, 1, t.hi, t.dhi);                        // g1a = h1b, g1b = h1a: colifilt(X, g1b, g1a, True)
    dtcwt_ifilt_taps(h2a, h2b, m, 1, t.ba, t.dba);                        // g2a = h2b, g2b = h2a: colifilt(X, g2b, g2a, True)
    return run_bwd_j2<true>("scat_bwd_j2_bp", dlow, dlow_sn, dlow_sc, dmag, dmag_sn, dmag_so, dmag_sc, phase, dx, N, C, H, W, m, t, stream);
}
