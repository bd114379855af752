// 1-D filter-bank DWT / IDWT over rows, every level of a row in ONE launch, fp32 (pytorch_wavelets dwt/transform1d.py:7-115
// DWT1DForward / DWT1DInverse, dwt/lowlevel.py:368-424 AFB1D, 697-743 SFB1D).  Any even tap count 2 <= L <= 16, one bank, the
// padding modes zero, symmetric, reflect, periodic and periodization, 1 <= J <= 8 levels.  The per-level arithmetic is the
// 1-D half of what dwt.hip documents:
//
// Analysis, per level, n samples in, O out:   out[i] = sum_k h[k] * xe[2 i + k - base]
//   O = (n + L - 1) / 2, base = p / 2, p = 2 (O - 1) - n + L, xe the mode's extension of x (folded or wrapped as often as the
//   position asks: 'reflect' works at lengths where F.pad refuses)                                        (zero .. periodic)
//   O = (n + 1) / 2, base = L - 1, xe[j] = x[min(((j mod Ne) + L/2) mod Ne, n - 1)] for -Ne <= j < Ne, 0 elsewhere,
//   Ne = n + (n & 1)                                                                                       (periodization)
// A level j > 0 may be told to read ONE sample more than level j - 1 produced: that sample is a zero, appended before the
// extension (DWT1DInverse's backward: the sample the inverse dropped from its running lowpass gets a zero gradient).
//
// Synthesis, per level, n coefficients in:    full[m] = sum_i lo[i] g0[m - 2 i] + hi[i] g1[m - 2 i]
//   y[t] = full[t + L - 2], 0 <= t < 2 n - L + 2                                                           (zero .. periodic)
//   y[t] = w[(t + L/2 - 1) mod 2n], w[u] = full[u] + (u < L - 2 ? full[u + 2n] : 0), 2 n outputs           (periodization)
// written, as in dwt.hip, as one transposed bank over a virtual coefficient index i' that wraps (c[i' mod n]): i' in [-n, n)
// for u' = t + L/2 - 1 < 2n and in [0, 2n) beyond; the other modes use i' in [0, n) and u' = t + L - 2.  Levels run from the
// coarsest to the finest; level j's result is cropped to the next level's coefficient count, the finest to out_len.
//
// fb_map (the extension's index map) and fb_syn_out of filterbank_dev.h, shared with dwt.hip, and dwt1d_ana_out (one output:
// explicit fmaf, taps k = 0 .. L-1 in order) serve every launch shape, so a coefficient has the same bits whatever block, tile
// or launch computed it.
//
// Launch shapes.  FUSED: a workgroup of 256 threads owns R rows (R = 1 for a long row, a power of two up to 16 for short
// ones, 256 / R lanes per row) and runs level after level between two LDS buffers: E, the level's extended input (the index
// map is applied once per sample while E is filled -- from global memory for level 0, from P afterwards), and P, the level's
// lowpass.  Each level's hi and the last lo go to global memory; x is read once, every coefficient written once, nothing
// intermediate leaves the CU.  The synthesis keeps A and H (the level's lo and hi, as a patch of virtual coefficient indices)
// and P (its result, the next level's lo); the finest level stores to global memory.  TILED, for rows too long for LDS: the
// same kernel body with J = 1 and one tile of a level's outputs per workgroup (DWT1D_TA analysis outputs with the L - 2
// halo, DWT1D_TS synthesis outputs with L/2 coefficients of halo), one launch per level, the lowpass travelling through
// global memory.  The taps, the per-level lengths and the J hi pointers travel by value in the kernel arguments: no device
// allocation, no copy, no state -- either launch can be captured in a graph.
//
// The fused limit, DWT1D_FUSED_MAX = 8192 samples a row.  A workgroup may declare all 160 KiB of a CU's LDS, which would hold a
// row of ~27000 samples with its half-length second buffer -- as ONE workgroup of 4 waves on the CU, far too few to cover the
// HBM latency of a kernel that is a stream (8 bytes of traffic per sample against ~2 L flops).  At 8192 the analysis needs
// (8192 + 32) + (4096 + 9) floats = 48.2 KiB and the synthesis 3 (4096 + 24) floats = 48.3 KiB: three workgroups, 12 waves,
// per CU, each in a different phase (loading, filtering, storing), and below the 64 KiB that need no opt-in.  The LDS is
// declared dynamically at what the rows of the call need, so shorter rows get more workgroups per CU, up to the wave limit.
// Beyond 8192 the tiles (16.4 KiB) keep that occupancy at any length.
//
// LDS banks.  The analysis reads xe at stride 2 across lanes: as 4-byte reads (32 banks) that is a 2-way conflict on every
// read.  E therefore stores the EXTENDED signal from position -base on, E[e] = xe[e - base], which makes the window of output
// i start at the even offset 2 i whatever the parity of base: a lane reads its window as L/2 aligned float2 (ds_read_b64, 64
// banks, 32 lanes x 8 bytes = one bank row: conflict-free), rows of E an even number of floats apart.  The synthesis would
// write interleaved (even / odd phase) if a lane produced a coefficient's two outputs; instead a lane owns ONE output t,
// lanes run along t: the stores (LDS and global) are consecutive, and the loads see lanes 2 m and 2 m + 1 on the same
// coefficient (a broadcast), 32 lanes on 16 or 17 consecutive words -- no conflict.  The even / odd lanes pick their taps
// (g[2 q] or g[2 q + 1]) by a select between two scalars.  All fills and P accesses are consecutive.
#include <cstdint>
#include "filterbank_dev.h"

namespace faoctasr {

constexpr int DWT1D_MAXJ = 8;
constexpr int DWT1D_FUSED_MAX = 8192;
constexpr int DWT1D_TA = 2048;                  // tiled analysis: outputs per workgroup
constexpr int DWT1D_TS = 4096;                  // tiled synthesis: outputs per workgroup

struct Dwt1dPtrs { float* p[DWT1D_MAXJ]; };
struct Dwt1dLens { int n[DWT1D_MAXJ], src[DWT1D_MAXJ]; };   // analysis: logical / real input length; synthesis: count / crop
// rows of an operand: row r starts at (r / inner) * outer + (r % inner) * step elements (an (N, C, n) tensor with last stride 1)
struct Dwt1dRows { long inner, outer, step; };

// one analysis output from its window w = &E[2 i] (8-byte aligned): taps k = 0 .. L-1 in order
__device__ __forceinline__ void dwt1d_ana_out(const float* w, int L, const FbTaps1& taps, float& lo, float& hv) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < L; k += 2) {
        const float2 v = *reinterpret_cast<const float2*>(w + k);
        a = fmaf(taps.f0[k], v.x, a);
        b = fmaf(taps.f1[k], v.x, b);
        a = fmaf(taps.f0[k + 1], v.y, a);
        b = fmaf(taps.f1[k + 1], v.y, b);
    }
    lo = a;
    hv = b;
}

__device__ __forceinline__ int d1_out_size(int n, int L, bool per) { return per ? (n + 1) >> 1 : (n + L - 1) >> 1; }

// shift = log2(R): lanes (tid >> (8 - shift)) ... own row r of the block, 256 >> shift lanes a row
__global__ __launch_bounds__(256) void dwt1d_analysis_kernel(const float* __restrict__ x, Dwt1dRows xr, float* __restrict__ lo, Dwt1dPtrs hi,
                                                             long NC, int J, int shift, int tiles, int T, int ecap, int pcap, int L,
                                                             int mode, Dwt1dLens len, FbTaps1 taps) {
    extern __shared__ __attribute__((aligned(16))) float d1_smem[];
    const int R = 1 << shift, tpr = 256 >> shift;
    const int r = threadIdx.x >> (8 - shift), c0 = threadIdx.x & (tpr - 1);
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const long row = (long)(blockIdx.x / (unsigned)tiles) * R + r;
    const bool live = row < NC;
    float* E = d1_smem + (size_t)r * ecap;
    float* P = d1_smem + (size_t)R * ecap + (size_t)r * pcap;
    const float* xp = live ? x + (row / xr.inner) * xr.outer + (row % xr.inner) * xr.step : x;
    const bool per = mode == MODE_PER;

    for (int j = 0; j < J; ++j) {
        const int n = len.n[j], ns = len.src[j];
        const int O = d1_out_size(n, L, per);
        const int base = per ? L - 1 : (2 * (O - 1) - n + L) >> 1;
        const int o0 = tile * T;
        const int cnt = min(T, O - o0);
        const int elen = 2 * (cnt - 1) + L;                 // <= ecap
        if (live) {
            const int p0 = 2 * o0 - base;
            if (j == 0) {
                for (int e = c0; e < elen; e += tpr) {
                    const int s = fb_map(p0 + e, n, mode, L >> 1);
                    E[e] = (s >= 0 && s < ns) ? xp[s] : 0.f;
                }
            } else {
                for (int e = c0; e < elen; e += tpr) {
                    const int s = fb_map(p0 + e, n, mode, L >> 1);
                    E[e] = (s >= 0 && s < ns) ? P[s] : 0.f;
                }
            }
        }
        __syncthreads();
        if (live) {
            float* hp = hi.p[j] + row * (long)O + o0;
            float* lp = lo + row * (long)O + o0;
            const bool last = j == J - 1;
            for (int c = c0; c < cnt; c += tpr) {
                float l, h;
                dwt1d_ana_out(E + 2 * c, L, taps, l, h);
                hp[c] = h;
                if (last) lp[c] = l; else P[c] = l;
            }
        }
        __syncthreads();
    }
}

// len.n[j]: coefficient count of level j; len.src[j]: the length level j's result is cropped to (src[0] = out_len)
__global__ __launch_bounds__(256) void dwt1d_synthesis_kernel(const float* __restrict__ lo, Dwt1dRows lr, Dwt1dPtrs hi, float* __restrict__ y,
                                                              long NC, int J, int shift, int tiles, int T, int acap, int pcap, int L,
                                                              int mode, Dwt1dLens len, FbTaps1 taps) {
    extern __shared__ __attribute__((aligned(16))) float d1_smem[];
    const int R = 1 << shift, tpr = 256 >> shift;
    const int r = threadIdx.x >> (8 - shift), c0 = threadIdx.x & (tpr - 1);
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const long row = (long)(blockIdx.x / (unsigned)tiles) * R + r;
    const bool live = row < NC;
    float* A = d1_smem + (size_t)r * acap;
    float* H = d1_smem + (size_t)R * acap + (size_t)r * acap;
    float* P = d1_smem + (size_t)2 * R * acap + (size_t)r * pcap;
    const float* lp = live ? lo + (row / lr.inner) * lr.outer + (row % lr.inner) * lr.step : lo;
    const bool per = mode == MODE_PER;
    const int off = per ? (L >> 1) - 1 : L - 2;

    for (int j = J - 1; j >= 0; --j) {
        const int n = len.n[j], crop = len.src[j];
        const int t0 = tile * T;
        const int cnt = min(T, crop - t0);
        const int ib = (t0 + off - L + 2) >> 1;                             // first virtual coefficient (floor)
        const int pc = ((t0 + cnt - 1 + off) >> 1) - ib + 1;                // <= acap
        if (live) {
            const float* hp = hi.p[j] ? hi.p[j] + row * (long)n : nullptr;
            if (j == J - 1) {
                for (int e = c0; e < pc; e += tpr) A[e] = lp[pmod(ib + e, n)];
            } else {
                for (int e = c0; e < pc; e += tpr) A[e] = P[pmod(ib + e, n)];
            }
            for (int e = c0; e < pc; e += tpr) H[e] = hp ? hp[pmod(ib + e, n)] : 0.f;
        }
        __syncthreads();
        if (live) {
            float* yp = y + row * (long)crop + t0;
            for (int c = c0; c < cnt; c += tpr) {
                const float v = fb_syn_out(A, H, ib, n, t0 + c + off, per, L, taps);
                if (j == 0) yp[c] = v; else P[c] = v;
            }
        }
        __syncthreads();
    }
}

static int d1_check(const char* what, long NC, int J, int L, int mode, const float* a, const float* b) {
    if (!a || !b) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (NC < 1) return fail(FAOCTASR_EINVAL, "%s: NC %ld", what, NC);
    if (J < 1 || J > DWT1D_MAXJ) return fail(FAOCTASR_EINVAL, "%s: J %d outside 1..%d", what, J, DWT1D_MAXJ);
    if (!fb_len_ok(L)) return fail(FAOCTASR_EINVAL, "%s: tap count L %d must be even and within 2..%d", what, L, FB_MAXL);
    if (mode != MODE_ZERO && mode != MODE_SYMMETRIC && mode != MODE_PER && mode != MODE_REFLECT && mode != MODE_PERIODIC)
        return fail(FAOCTASR_EINVAL, "%s: unknown padding mode %d (0 zero, 1 symmetric, 2 periodization, 4 reflect, 6 periodic)", what, mode);
    return FAOCTASR_OK;
}

static int d1_rows_ok(const char* what, long inner, long outer, long step, long n) {
    if (inner < 1 || step < n || outer < 0) return fail(FAOCTASR_EINVAL, "%s: rows of %ld samples, %ld a group, strides %ld / %ld", what, n, inner, outer, step);
    return FAOCTASR_OK;
}

// log2 of the rows a fused workgroup owns: 256 / R lanes a row, about two level-0 outputs a lane, at least ~512 workgroups
static int d1_row_shift(long NC, int n) {
    int shift = 0;
    while (shift < 4 && ((long)n << (shift + 1)) <= 1024) ++shift;
    while (shift > 0 && ((NC + (1L << shift) - 1) >> shift) < 512) --shift;
    return shift;
}

}  // namespace faoctasr

using namespace faoctasr;

extern "C" long faoctasr_dwt1d_fused_max(void) { return DWT1D_FUSED_MAX; }

extern "C" int faoctasr_dwt1d_analysis(const float* x, long x_inner, long x_outer_stride, long x_row_stride, float* lo, float* const* hi,
                                       long NC, int n, const int* in_lens, int J, const float* h0, const float* h1, int L, int mode,
                                       int fused, faoctasr_stream_t stream) {
    int rc = d1_check("dwt1d_analysis", NC, J, L, mode, h0, h1);
    if (rc) return rc;
    if (!x || !lo || !hi) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: null pointer");
    if (n < 1) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: n %d", n);
    if ((rc = d1_rows_ok("dwt1d_analysis", x_inner, x_outer_stride, x_row_stride, n))) return rc;
    if (!fused && J != 1) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: the tiled launch runs one level a call, got J %d", J);
    const bool per = mode == MODE_PER;
    Dwt1dLens len = {};
    Dwt1dPtrs hp = {};
    int have = n, nmax = 0, omax = 0;                       // samples the level's source holds
    for (int j = 0; j < J; ++j) {
        const int want = in_lens ? in_lens[j] : have;
        if (want != have && want != have + 1)
            return fail(FAOCTASR_EINVAL, "dwt1d_analysis: level %d is to read %d samples of a source that holds %d (that, or one zero more)", j, want, have);
        if (want < 2) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: level %d has %d samples, below the minimum 2", j, want);
        if (!hi[j]) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: null hi pointer at level %d", j);
        len.n[j] = want;
        len.src[j] = have;
        hp.p[j] = hi[j];
        if (want > nmax) nmax = want;
        have = per ? (want + 1) / 2 : (want + L - 1) / 2;
        if (have > omax) omax = have;
    }
    const int O0 = per ? (len.n[0] + 1) / 2 : (len.n[0] + L - 1) / 2;
    int shift = 0, tiles = 1, T = 1 << 30, ecap, pcap;      // fused: one "tile" holds any level (a short row's levels can grow: O > n below L - 1)
    if (fused) {
        if (n > DWT1D_FUSED_MAX) return fail(FAOCTASR_EINVAL, "dwt1d_analysis: a row of %d samples is beyond the fused launch's %d", n, DWT1D_FUSED_MAX);
        shift = d1_row_shift(NC, n);
        ecap = (nmax + 2 * L + 1) & ~1;                     // 2 (O - 1) + L <= n + 2 L - 3, even: float2 windows in every row
        pcap = omax + 1;
    } else {
        T = DWT1D_TA;
        tiles = (O0 + T - 1) / T;
        ecap = 2 * T + L;
        pcap = 0;
    }
    const long groups = (NC + (1L << shift) - 1) >> shift;
    if (groups > 0x7fffffffL / tiles) return fail(FAOCTASR_EUNSUPPORTED, "dwt1d_analysis: NC %ld n %d needs more than 2^31 - 1 blocks", NC, n);
    const size_t lds = ((size_t)(ecap + pcap) << shift) * sizeof(float);
    hipLaunchKernelGGL(dwt1d_analysis_kernel, dim3((unsigned)(groups * tiles)), dim3(256), lds, (hipStream_t)stream, x,
                       Dwt1dRows{x_inner, x_outer_stride, x_row_stride}, lo, hp, NC, J, shift, tiles, T, ecap, pcap, L, mode, len, fb_taps1(h0, h1, L));
    return check_launch("dwt1d_analysis");
}

extern "C" int faoctasr_dwt1d_synthesis(const float* lo, long lo_inner, long lo_outer_stride, long lo_row_stride, const float* const* hi,
                                        float* y, long NC, const int* counts, int J, int out_len, const float* g0, const float* g1, int L,
                                        int mode, int fused, faoctasr_stream_t stream) {
    int rc = d1_check("dwt1d_synthesis", NC, J, L, mode, g0, g1);
    if (rc) return rc;
    if (!lo || !hi || !y || !counts) return fail(FAOCTASR_EINVAL, "dwt1d_synthesis: null pointer");
    if (!fused && J != 1) return fail(FAOCTASR_EINVAL, "dwt1d_synthesis: the tiled launch runs one level a call, got J %d", J);
    const bool per = mode == MODE_PER;
    Dwt1dLens len = {};
    Dwt1dPtrs hp = {};
    int nmax = 0;
    for (int j = 0; j < J; ++j) {
        const int c = counts[j];
        // a result of at least one sample (2 n - L + 2 >= 2), resp. a periodization roll of at most one turn (2 n >= L / 2)
        if (c < (per ? (L + 3) / 4 : L / 2)) return fail(FAOCTASR_EINVAL, "dwt1d_synthesis: %d coefficients at level %d, below the minimum (L %d)", c, j, L);
        const int full = per ? 2 * c : 2 * c - L + 2;
        const int crop = j ? counts[j - 1] : out_len;
        if (crop < 1 || crop > full) return fail(FAOCTASR_EINVAL, "dwt1d_synthesis: level %d's crop %d outside its result of %d", j, crop, full);
        len.n[j] = c;
        len.src[j] = crop;
        hp.p[j] = const_cast<float*>(hi[j]);
        if (c > nmax) nmax = c;
    }
    if ((rc = d1_rows_ok("dwt1d_synthesis", lo_inner, lo_outer_stride, lo_row_stride, counts[J - 1]))) return rc;
    int shift = 0, tiles = 1, T = 1 << 30, acap, pcap;
    if (fused) {
        if (out_len > DWT1D_FUSED_MAX) return fail(FAOCTASR_EINVAL, "dwt1d_synthesis: a row of %d samples is beyond the fused launch's %d", out_len, DWT1D_FUSED_MAX);
        shift = d1_row_shift(NC, out_len);
        acap = nmax + L;                                    // the patch: n + L/2 + 1 at most
        pcap = 0;                                           // the intermediate results: level j >= 1's, cropped to counts[j - 1]
        for (int j = 1; j < J; ++j) if (len.src[j] + 1 > pcap) pcap = len.src[j] + 1;
    } else {
        T = DWT1D_TS;
        tiles = (out_len + T - 1) / T;
        acap = T / 2 + L;
        pcap = 0;
    }
    const long groups = (NC + (1L << shift) - 1) >> shift;
    if (groups > 0x7fffffffL / tiles) return fail(FAOCTASR_EUNSUPPORTED, "dwt1d_synthesis: NC %ld out_len %d needs more than 2^31 - 1 blocks", NC, out_len);
    const size_t lds = ((size_t)(2 * acap + pcap) << shift) * sizeof(float);
    hipLaunchKernelGGL(dwt1d_synthesis_kernel, dim3((unsigned)(groups * tiles)), dim3(256), lds, (hipStream_t)stream, lo,
                       Dwt1dRows{lo_inner, lo_outer_stride, lo_row_stride}, hp, y, NC, J, shift, tiles, T, acap, pcap, L, mode, len, fb_taps1(g0, g1, L));
    return check_launch("dwt1d_synthesis");
}
