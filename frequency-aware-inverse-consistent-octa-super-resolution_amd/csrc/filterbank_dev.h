// What the filter-bank transforms share (dwt.hip, dwt1d.hip, swt.hip): the padding modes, the extension's index map, the taps as
// kernel arguments with their host-side checks, and the transposed-bank synthesis output.  One definition each, so a coefficient
// has the same bits whichever kernel computed it.
#pragma once
#include "common.h"

namespace faoctasr {

constexpr int FB_MAXL = 16;                     // taps per filter
constexpr int MODE_ZERO = 0, MODE_SYMMETRIC = 1, MODE_PER = 2, MODE_REFLECT = 4, MODE_PERIODIC = 6;      // pytorch_wavelets' mode numbers

// the taps travel by value: one bank (lo f0, hi f1) for a 1-D transform, two for a 2-D one (w along W, h along H)
struct FbTaps1 { float f0[FB_MAXL], f1[FB_MAXL]; };
struct FbTaps2 { FbTaps1 w, h; };

__device__ __forceinline__ int pmod(int j, int P) {
    const int m = j % P;
    return m < 0 ? m + P : m;
}

// index of the sample that position j of the extended signal reads, -1 for a zero; L2 = L / 2 (periodization only)
__device__ __forceinline__ int fb_map(int j, int N, int mode, int L2) {
    if (mode != MODE_PER && j >= 0 && j < N) return j;
    switch (mode) {
        case MODE_SYMMETRIC: { const int m = pmod(j, 2 * N); return m < N ? m : 2 * N - 1 - m; }          // fold about -1/2 and N-1/2
        case MODE_REFLECT: { if (N == 1) return 0; const int m = pmod(j, 2 * N - 2); return m < N ? m : 2 * N - 2 - m; }   // about 0 and N-1
        case MODE_PERIODIC: return pmod(j, N);
        case MODE_PER: {
            const int Ne = N + (N & 1);
            if (j < -Ne || j >= Ne) return -1;
            const int m = ((j < 0 ? j + Ne : j) + L2) % Ne;
            return m < N ? m : N - 1;
        }
        default: return -1;
    }
}

// one synthesis output at the unwrapped position u from the patches A (lo) and H (hi), whose entry 0 is virtual coefficient ib
__device__ __forceinline__ float fb_syn_out(const float* A, const float* H, int ib, int n, int u, bool per, int L, const FbTaps1& g) {
    const int lo_i = (per && u < 2 * n) ? -n : 0, hi_i = (per && u >= 2 * n) ? 2 * n : n;
    const bool odd = u & 1;
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < (L >> 1); ++q) {
        const int i = (u >> 1) - q;
        if (i < lo_i || i >= hi_i) continue;
        const float t0 = odd ? g.f0[2 * q + 1] : g.f0[2 * q], t1 = odd ? g.f1[2 * q + 1] : g.f1[2 * q];
        a0 = fmaf(A[i - ib], t0, a0);
        a1 = fmaf(H[i - ib], t1, a1);
    }
    return a0 + a1;
}

inline bool fb_len_ok(int L) { return L >= 2 && L <= FB_MAXL && !(L & 1); }

// what a 2-D entry point checks first: the four tap pointers, the plane count, an even tap count within 2..FB_MAXL per axis
inline int fb_check2(const char* what, long NC, int L_h, int L_w, const float* a, const float* b, const float* c, const float* d) {
    if (!a || !b || !c || !d) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (NC < 1) return fail(FAOCTASR_EINVAL, "%s: NC %ld", what, NC);
    if (!fb_len_ok(L_h) || !fb_len_ok(L_w))
        return fail(FAOCTASR_EINVAL, "%s: tap counts L_h %d L_w %d must be even and within 2..%d", what, L_h, L_w, FB_MAXL);
    return FAOCTASR_OK;
}

inline FbTaps1 fb_taps1(const float* f0, const float* f1, int L) {
    FbTaps1 t = {};
    for (int k = 0; k < L; ++k) { t.f0[k] = f0[k]; t.f1[k] = f1[k]; }
    return t;
}

inline FbTaps2 fb_taps2(const float* lo_h, const float* hi_h, int L_h, const float* lo_w, const float* hi_w, int L_w) {
    return FbTaps2{fb_taps1(lo_w, hi_w, L_w), fb_taps1(lo_h, hi_h, L_h)};
}

}  // namespace faoctasr
