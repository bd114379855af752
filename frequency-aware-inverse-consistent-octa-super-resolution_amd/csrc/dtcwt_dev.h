// What the dual-tree kernels of dtcwt.hip and the scattering kernels of scat.hip share: tap structs, tile constants, the
// extension's index map, q2c / c2q, and the host-side argument checks and synthesis tap table.  Notation and index maps: the
// head of dtcwt.hip.
#pragma once
#include <cstdint>
#include "common.h"

namespace faoctasr {

constexpr int DT_MAXL = 20;                       // level 1: odd 3..19; q-shift: even 4..20
constexpr float DT_S = 0.70710678118654752440f;

struct DtStr { long n, c, o, r, w, i; };         // bandpass element strides
struct DtLow { long n, c, r; };                  // lowpass input element strides

struct DtTaps1 { float f0[DT_MAXL], f1[DT_MAXL]; };                      // level 1: lowpass, highpass
struct DtTaps2 { float lo0[DT_MAXL], lo1[DT_MAXL], hi0[DT_MAXL], hi1[DT_MAXL]; };   // level >= 2 analysis, by output phase
struct DtTapsI { float lo[4][DT_MAXL / 2], hi[4][DT_MAXL / 2]; int dlo[4], dhi[4]; };   // level >= 2 synthesis, by output phase q
// the three-filter (rotationally symmetric, "_bp") banks: the two-filter taps and the bandpass filter of the diagonal band hh
struct DtTaps1R : DtTaps1 { float f2[DT_MAXL]; int L2; };               // level 1: + bandpass, of its own odd length
struct DtTaps2R : DtTaps2 { float ba0[DT_MAXL], ba1[DT_MAXL]; };        // level >= 2 analysis: + the bandpass pair, phased as hi0, hi1
struct DtTapsIR : DtTapsI { float ba[4][DT_MAXL / 2]; int dba[4]; };    // level >= 2 synthesis: + a third (highpass-call) table
// the tap structs of a kernel's two-filter (BP = false) and three-filter (BP = true) form
template <bool BP> struct DtBank { using T1 = DtTaps1; using T2 = DtTaps2; using TI = DtTapsI; };
template <> struct DtBank<true> { using T1 = DtTaps1R; using T2 = DtTaps2R; using TI = DtTapsIR; };

// level-1 tiles (forward: of ll; inverse: of y) and the level >= 2 ones (forward: of ll = 4 x 32 quads; inverse: of y)
constexpr int J1_TH = 16, J1_TW = 64, J1_PR = J1_TH + DT_MAXL - 2, J1_PC = J1_TW + DT_MAXL - 2;          // halo 2 * 9
constexpr int F2_TH = 8, F2_TW = 64, F2_PR = 2 * F2_TH + 2 * DT_MAXL - 4, F2_PC = 2 * F2_TW + 2 * DT_MAXL - 4;
constexpr int I2_TH = 32, I2_TW = 64, I2_PR = I2_TH / 2 + DT_MAXL, I2_PC = I2_TW / 2 + DT_MAXL;

// level-1 halo: the largest half-length of the bank's filters
template <bool BP>
__device__ __forceinline__ int dt_halo1(int L0, int L1, const typename DtBank<BP>::T1& taps) {
    int L = L0 > L1 ? L0 : L1;
    if constexpr (BP) L = taps.L2 > L ? taps.L2 : L;
    return L >> 1;
}

// index of the sample that position j of the extension reads; -1 for a zero
__device__ __forceinline__ int dt_map(int j, int N, int sym) {
    if (sym) {
        int m = j % (2 * N);
        if (m < 0) m += 2 * N;
        return m < N ? m : 2 * N - 1 - m;
    }
    return (j >= 0 && j < N) ? j : -1;
}

__device__ __forceinline__ void dt_put(float* p, long si, bool vec, float re, float im) {
    if (vec) *reinterpret_cast<float2*>(p) = make_float2(re, im);
    else { p[0] = re; p[si] = im; }
}

// q2c of one quad (top = a, b; bot = c, d): z1 = (a - d) + i (b + c), z2 = (a + d) + i (b - c), scaled by 1/sqrt 2 first
__device__ __forceinline__ void dt_q2c_val(float2 top, float2 bot, float2* z1, float2* z2) {
    const float a = top.x * DT_S, b = top.y * DT_S, c = bot.x * DT_S, d = bot.y * DT_S;
    *z1 = make_float2(a - d, b + c);
    *z2 = make_float2(a + d, b - c);
}

// q2c of one quad into orientations o1 (z1) and o2 (z2)
__device__ __forceinline__ void dt_q2c(float* q, const DtStr& s, bool vec, int o1, int o2, float2 top, float2 bot) {
    float2 z1, z2;
    dt_q2c_val(top, bot, &z1, &z2);
    dt_put(q + o1 * s.o, s.i, vec, z1.x, z1.y);
    dt_put(q + o2 * s.o, s.i, vec, z2.x, z2.y);
}

// c2q: the value at row parity pr, column parity pc of the quad whose complex pair has the components w1, w2 that the parities
// select ((0,1) and (1,0) take the imaginary parts, the other two the real ones)
__device__ __forceinline__ float dt_c2q_val(float w1, float w2, int pr, int pc) {
    return (pr ? (pc ? w2 - w1 : w1 - w2) : w1 + w2) * DT_S;
}

// c2q: the value at row parity pr, column parity pc of the quad whose complex pair (w1, w2) starts at p1, p2
__device__ __forceinline__ float dt_c2q(const float* p1, const float* p2, long si, int pr, int pc) {
    const long comp = (pr ^ pc) ? si : 0;                   // (0,1) and (1,0) read the imaginary parts
    return dt_c2q_val(p1[comp], p2[comp], pr, pc);
}

// stage one coefficient position (sr, sc) of the four full-resolution planes ll, lh, hl, hh (c2q applied on the way)
__device__ __forceinline__ void dt_stage(const float* lp, DtLow ls, const float* hp, const DtStr& hs, int sr, int sc, float* o0, float* o1,
                                         float* o2, float* o3) {
    *o0 = lp ? lp[sr * ls.r + sc] : 0.f;
    if (hp) {
        const float* q = hp + (long)(sr >> 1) * hs.r + (long)(sc >> 1) * hs.w;
        const int pr = sr & 1, pc = sc & 1;
        *o1 = dt_c2q(q, q + 5 * hs.o, hs.i, pr, pc);                      // lh: 15, 165
        *o2 = dt_c2q(q + 2 * hs.o, q + 3 * hs.o, hs.i, pr, pc);           // hl: 75, 105
        *o3 = dt_c2q(q + hs.o, q + 4 * hs.o, hs.i, pr, pc);               // hh: 45, 135
    } else {
        *o1 = *o2 = *o3 = 0.f;
    }
}

inline int dt_blocks(const char* what, long N, int C, int tiles_h, int tiles_w, long* blocks) {
    if (N < 1 || C < 1) return fail(FAOCTASR_EINVAL, "%s: N %ld C %d", what, N, C);
    *blocks = N * C * tiles_h * (long)tiles_w;
    if (*blocks > 0x7fffffffL) return fail(FAOCTASR_EUNSUPPORTED, "%s: N %ld C %d needs more than 2^31 - 1 blocks", what, N, C);
    return FAOCTASR_OK;
}

inline int dt_taps1(const char* what, const float* f0, int L0, const float* f1, int L1, DtTaps1* t) {
    if (!f0 || !f1) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (L0 < 3 || L0 >= DT_MAXL || !(L0 & 1) || L1 < 3 || L1 >= DT_MAXL || !(L1 & 1))
        return fail(FAOCTASR_EINVAL, "%s: level-1 tap counts %d and %d must be odd and within 3..%d", what, L0, L1, DT_MAXL - 1);
    *t = DtTaps1{};
    for (int k = 0; k < L0; ++k) t->f0[k] = f0[k];
    for (int k = 0; k < L1; ++k) t->f1[k] = f1[k];
    return FAOCTASR_OK;
}

// the third level-1 filter joins a checked two-filter set
inline int dt_taps1r(const char* what, const float* f0, int L0, const float* f1, int L1, const float* f2, int L2, DtTaps1R* t) {
    DtTaps1 two;
    const int rc = dt_taps1(what, f0, L0, f1, L1, &two);
    if (rc) return rc;
    if (!f2) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (L2 < 3 || L2 >= DT_MAXL || !(L2 & 1))
        return fail(FAOCTASR_EINVAL, "%s: level-1 third-filter tap count %d must be odd and within 3..%d", what, L2, DT_MAXL - 1);
    *t = DtTaps1R{};
    static_cast<DtTaps1&>(*t) = two;
    for (int k = 0; k < L2; ++k) t->f2[k] = f2[k];
    t->L2 = L2;
    return FAOCTASR_OK;
}

inline int dt_taps2_check(const char* what, const float* a, const float* b, const float* c, const float* d, int m) {
    if (!a || !b || !c || !d) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    if (m < 4 || m > DT_MAXL || (m & 1)) return fail(FAOCTASR_EINVAL, "%s: q-shift tap count %d must be even and within 4..%d", what, m, DT_MAXL);
    return FAOCTASR_OK;
}

inline int dt_taps2r_check(const char* what, const float* a, const float* b, const float* c, const float* d, const float* e, const float* f,
                           int m) {
    if (!e || !f) return fail(FAOCTASR_EINVAL, "%s: null tap pointer", what);
    return dt_taps2_check(what, a, b, c, d, m);
}

// analysis taps by output phase: the lowpass call reads (h0b, h0a), the highpass calls (h1a, h1b) and (h2a, h2b)
inline void dt_taps2_fill(DtTaps2* t, const float* h0a, const float* h0b, const float* h1a, const float* h1b, int m) {
    for (int k = 0; k < m; ++k) { t->lo0[k] = h0b[k]; t->lo1[k] = h0a[k]; t->hi0[k] = h1a[k]; t->hi1[k] = h1b[k]; }
}
inline void dt_taps2_fill(DtTaps2R* t, const float* h0a, const float* h0b, const float* h1a, const float* h1b, const float* h2a,
                          const float* h2b, int m) {
    dt_taps2_fill(static_cast<DtTaps2*>(t), h0a, h0b, h1a, h1b, m);
    for (int k = 0; k < m; ++k) { t->ba0[k] = h2a[k]; t->ba1[k] = h2b[k]; }
}

// the table of lowlevel.py:154-239: per output phase q the polyphase half and offset of colifilt(X, fa, fb, highpass)
inline void dtcwt_ifilt_taps(const float* fa, const float* fb, int m, int highpass, float out[4][DT_MAXL / 2], int d[4]) {
    const int m2 = m / 2;
    // which filter (0 = fa, 1 = fb), which half (0 = even taps, 1 = odd taps), offset
    static const int even_lo[4][3] = {{0, 0, 0}, {1, 0, 1}, {0, 1, 2}, {1, 1, 3}}, even_hi[4][3] = {{0, 0, 1}, {1, 0, 0}, {0, 1, 3}, {1, 1, 2}};
    static const int odd_lo[4][3] = {{0, 1, 1}, {1, 1, 2}, {0, 0, 1}, {1, 0, 2}}, odd_hi[4][3] = {{0, 1, 2}, {1, 1, 1}, {0, 0, 2}, {1, 0, 1}};
    const int (*tab)[3] = (m2 & 1) ? (highpass ? odd_hi : odd_lo) : (highpass ? even_hi : even_lo);
    for (int q = 0; q < 4; ++q) {
        const float* f = tab[q][0] ? fb : fa;
        for (int t = 0; t < DT_MAXL / 2; ++t) out[q][t] = t < m2 ? f[2 * t + tab[q][1]] : 0.f;
        d[q] = tab[q][2];
    }
}

}  // namespace faoctasr
