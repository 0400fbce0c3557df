// tuner_host.hpp -- host-side (plain C++, no HIP) arithmetic of the wideband tuner (tuner.hip, kernels_tuner.hip,
// kernels_tuner_rational.hip): frequency word, complex integer taps per phase, the rotation table, and the matrix-core
// operand image of a channel group.  One of each, for every rate U / D: the integer tuner is U = 1.
// Header-only, like fe_mfma_host.hpp.  The arithmetic is DEFINED by tests/_tuner_model.py and, for U > 1,
// tests/_tuner_rational_model.py (DESIGN.md sections 4.9 and 4.9.2); this file is the product's statement of it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace fmrx {

constexpr int kTunerTableBits = 12;                  // rotation table: 2^12 entries of round(32767 cos), round(32767 sin)
constexpr int kTunerTableSize = 1 << kTunerTableBits;
constexpr int kTunerDigits = 2;                      // balanced base-256 digits of a tap part
constexpr double kTunerTapLimit = 127.0 * 256.0;     // max |re|, |im| of a scaled tap: both balanced digits of +q and -q fit int8
constexpr int kTunerMinShift = -14, kTunerMaxShift = 47;   // range of s: the output shift s + 15 stays in 1 .. 62
constexpr int kTunerMaxR = 32, kTunerMaxTaps = 4096;
constexpr int kTunerMfmaMaxTaps = 256;               // the matrix kernel's operand image grows with T; longer filters run the generic kernel
constexpr int kTunerPhases = 8;                      // consecutive outputs per MFMA column (16 bytes of a channel's row)
constexpr int kTunerGroup = 4;                       // channels per MFMA tile: 4 rows each (re / im x 2 digits)
constexpr double kTunerTwoPi = 6.283185307179586476925286766559;

// Input formats (include/fmrx.h: FMRX_TUNER_U8 / S8 / S16; arithmetic defined by tests/_tuner_formats_model.py).  A wide
// sample is an (I, Q) pair of values: x = u8 - 128, the int8, or the little-endian int16.  A format carries B extra bits of
// input scale (the output shift is s + 15 + B, so unity gain maps full scale in to full scale out); the "zero sample" in
// front of a stream and past a call is the value whose x is 0.
constexpr int kTunerU8 = 0, kTunerS8 = 1, kTunerS16 = 2;
inline bool tuner_format_ok(int f) { return f == kTunerU8 || f == kTunerS8 || f == kTunerS16; }
inline int tuner_value_bytes(int f) { return f == kTunerS16 ? 2 : 1; }          // bytes per I or Q value
inline int tuner_extra_bits(int f) { return f == kTunerS16 ? 8 : 0; }           // B
inline int tuner_zero_byte(int f) { return f == kTunerU8 ? 0x80 : 0x00; }       // every byte of a zero sample
inline int tuner_max_shift(int f) { return kTunerMaxShift - tuner_extra_bits(f); }   // largest s: s + 15 + B <= 62

// w = round(f_c / Fs_w * 2^32) mod 2^32 (half away from zero); |f_c| < Fs_w / 2 is the caller's to check
inline uint32_t tuner_freq_word(double f_c, double Fs_w)
{
    const double v = f_c / Fs_w * 4294967296.0;
    const long long r = std::llround(v);
    return static_cast<uint32_t>(static_cast<unsigned long long>(r) & 0xffffffffULL);
}

// Rates: rf_Fs = Fs_w * U / D (DESIGN.md sections 4.9 and 4.9.2; arithmetic defined by tests/_tuner_rational_model.py, which
// at U = 1 is tests/_tuner_model.py).  Output m of the stream has n_m = floor(m D / U) as its newest wide sample and sums phase
// p_m = m D mod U of the prototype (designed at U * Fs_w, zero-padded to U * Tp taps, Tp = ceil(T / U)) over the Tp samples
// x[n_m - j].  U = 1 is plain decimation by D: one phase, the whole filter, n_m = m D.
constexpr int kTunerMaxU = 32, kTunerMaxD = 512;
constexpr int kTunerRatMfmaMaxU = 24, kTunerRatMfmaMaxD = 125;   // the range the matrix kernels cover (with Tp <= kTunerMfmaMaxTaps)

inline int tuner_gcd(int a, int b)
{
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    return a;
}
// error text of a ratio (nullptr = accepted)
inline const char *tuner_ratio_check(int U, int D)
{
    if (U < 1 || U > kTunerMaxU) return "U must be 1 .. 32";
    if (D < 2 * U || D > kTunerMaxD) return "D must be 2 U .. 512";
    if (tuner_gcd(U, D) != 1) return "U and D must have no common factor (gcd(U, D) = 1)";
    return nullptr;
}
inline int tuner_phase_taps(int T, int U) { return (T + U - 1) / U; }   // Tp
// the rates the integer matrix kernels (kernels_tuner.hip) are written for; every other rate runs the rational ones
inline bool tuner_integer_rate(int U, int D) { return U == 1 && D <= kTunerMaxR; }

// One channel's integers: tap (p, j) = gain h[p + j U] (cos a_j, sin a_j), a_j = 2 pi ((w j mod 2^32) / 2^32), ONE s for all
// phases, re / im phase-major [p * Tp + j] (U = 1: re[k], im[k] of tap k); the accumulator's worst case is per phase.  Returns
// the error text (nullptr = accepted).
inline const char *tuner_design(const float *h, int T, int U, double Fs_w, double f_c, double gain, uint32_t *w_out, int *s_out, int16_t *re,
                                int16_t *im)
{
    if (!h || T < 2 || T > kTunerMaxTaps) return "taps: 2 .. 4096";
    if (U < 1 || U > kTunerMaxU) return "U must be 1 .. 32";
    if (!(Fs_w > 0.0) || !std::isfinite(Fs_w)) return "Fs_w must be positive and finite";
    if (!std::isfinite(f_c) || !(std::fabs(f_c) < Fs_w / 2)) return "|f_c| must be below Fs_w / 2";
    if (!std::isfinite(gain)) return "gain must be finite";
    const uint32_t w = tuner_freq_word(f_c, Fs_w);
    const int Tp = tuner_phase_taps(T, U);
    const size_t n = static_cast<size_t>(U) * Tp;
    std::vector<double> gr(n, 0.0), gi(n, 0.0);
    double m = 0.0;
    for (int k = 0; k < T; k++) {
        if (!std::isfinite(h[k])) return "non-finite tap";
        const int p = k % U, j = k / U;
        const uint32_t ph = w * static_cast<uint32_t>(j);                       // w j mod 2^32
        const double a = kTunerTwoPi * (static_cast<double>(ph) / 4294967296.0);
        const double g = gain * static_cast<double>(h[k]);
        const size_t i = static_cast<size_t>(p) * Tp + j;
        gr[i] = g * std::cos(a);
        gi[i] = g * std::sin(a);
        m = std::fmax(m, std::fmax(std::fabs(gr[i]), std::fabs(gi[i])));
    }
    if (!std::isfinite(m) || m == 0.0) return "gain x taps are all zero or not finite";
    int s = static_cast<int>(std::floor(std::log2(kTunerTapLimit / m)));
    while (std::ldexp(m, s) > kTunerTapLimit) s--;
    while (std::ldexp(m, s + 1) <= kTunerTapLimit) s++;
    if (s < kTunerMinShift || s > kTunerMaxShift) return "gain x taps out of range (scale exponent outside -14 .. 47)";
    long long worst = 0;
    for (int p = 0; p < U; p++) {
        long long sum = 0;
        for (int j = 0; j < Tp; j++) {
            const size_t i = static_cast<size_t>(p) * Tp + j;
            const long long qr = std::llround(std::ldexp(gr[i], s)), qi = std::llround(std::ldexp(gi[i], s));
            re[i] = static_cast<int16_t>(qr);
            im[i] = static_cast<int16_t>(qi);
            sum += std::llabs(qr) + std::llabs(qi);
        }
        worst = std::max(worst, sum);
    }
    if (128 * worst > 2147483647LL) return "worst-case accumulator of a phase, 128 * sum(|re| + |im|), does not fit int32";
    *w_out = w;
    *s_out = s;
    return nullptr;
}

inline void tuner_table(int16_t *c, int16_t *s)
{
    for (int i = 0; i < kTunerTableSize; i++) {
        const double a = kTunerTwoPi * (static_cast<double>(i) / kTunerTableSize);
        c[i] = static_cast<int16_t>(std::llround(32767.0 * std::cos(a)));
        s[i] = static_cast<int16_t>(std::llround(32767.0 * std::sin(a)));
    }
}

// q = d0 + 256 d1, both digits in [-128, 127] (|q| <= 32512)
inline void tuner_digits(int q, int8_t *dig)
{
    const int d0 = ((q + 128) & 255) - 128;
    dig[0] = static_cast<int8_t>(d0);
    dig[1] = static_cast<int8_t>((q - d0) / 256);
}

// Shape of the matrix kernels' tile.  A column is 8 U consecutive outputs of every channel of the group; its window starts
// `front` bytes in front of the newest sample of its first output and 16 D bytes after its neighbour's.  Output q of the
// column (image q) has phase p_q = q D mod U and its newest sample floor(q D / U) samples into the column: window byte u
// meets tap j and part c (0 = I, 1 = Q) where  u = front + 2 floor(q D / U) - 2 j + c.  Image q's taps lie in the K-steps
// j0[q] .. j1[q]-1 (64 bytes each); only those are stored (ksp = the largest count) and multiplied.  At U = 1 the 8 images are
// the integer kernels' 8 phases: the same taps shifted by 2 D bytes each.
struct TunerShape {
    int U = 1, D = 2, Tp = 0;
    int front = 0;       // multiple of 16, >= 2 (Tp - 1) and >= 16
    int ks = 0;          // K-steps the whole window spans
    int ksp = 0;         // K-steps stored per image
    std::vector<int> j0, j1;   // [8 U]
};
inline TunerShape tuner_shape(int T, int U, int D)
{
    TunerShape s;
    s.U = U;
    s.D = D;
    s.Tp = tuner_phase_taps(T, U);
    s.front = std::max(16, (2 * (s.Tp - 1) + 15) / 16 * 16);   // Tp = 1 carries no history; the buffers keep one piece
    const int nq = kTunerPhases * U;
    s.j0.resize(nq);
    s.j1.resize(nq);
    for (int q = 0; q < nq; q++) {
        const int off = 2 * (q * D / U);
        s.j0[q] = (s.front + off - 2 * (s.Tp - 1)) / 64;
        s.j1[q] = (s.front + off + 1) / 64 + 1;
        s.ksp = std::max(s.ksp, s.j1[q] - s.j0[q]);
    }
    s.ks = s.j1[nq - 1];
    return s;
}
// LDS of a matrix kernel's workgroup: the rotation table, a step's window (`tiles` tiles of 16 columns per wave, 16 D bytes per
// column plus the reach, padded by one 16-byte piece per D; two byte planes for S16) and, with via_lds, the four waves' output
// buffers of tiles x 4 channels x 256 U bytes.
inline size_t tuner_lds_bytes(int U, int D, int ks, int format, int tiles, bool via_lds)
{
    const int planes = format == kTunerS16 ? 2 : 1;
    const int n_pieces = 16 * tiles * D + 4 * ks;
    return static_cast<size_t>(kTunerTableSize) * 4 + 16u * planes * (n_pieces + n_pieces / D + 1) +
           (via_lds ? static_cast<size_t>(4) * tiles * 4 * 256 * U : 0);
}
constexpr size_t kTwoPerCu = 64 * 1024;   // the most that leaves two workgroups on a CU, and what a kernel gets without asking for it
constexpr size_t kOnePerCu = 160 * 1024;  // LDS of a workgroup that has a CU to itself
constexpr int kTT = 4;                    // integer matrix kernels, 8-bit formats: tiles (of 16 columns x 8 outputs) per wave and step
constexpr int kTT16 = 2;                  // integer matrix kernel, S16: two planes of accumulators per tile
constexpr int kTunerWorkgroups = 2048;    // workgroups of a matrix kernel's launch: enough to fill the chip a few times over

// Tiles per wave and step, and whether the outputs go through the LDS buffer.  The integer kernels are compiled for kTT / kTT16
// tiles and store directly.  The rational ones, in order of preference: the buffer with the most tiles that keep two workgroups
// on a CU; the buffer with one tile and one workgroup per CU; direct stores, by the same two rules.  tiles = 0: the window does
// not fit the matrix kernel at all.
struct TunerPlan {
    int tiles;                           // 4, 2, 1, or 0 where the window does not fit the matrix kernel
    bool via_lds;
};
inline TunerPlan tuner_plan(int U, int D, int ks, int format)
{
    if (tuner_integer_rate(U, D)) return {format == kTunerS16 ? kTT16 : kTT, false};
    for (int via = 1; via >= 0; via--) {
        for (int tiles = format == kTunerS16 ? 2 : 4; tiles >= 1; tiles >>= 1)
            if (tuner_lds_bytes(U, D, ks, format, tiles, via) <= kTwoPerCu) return {tiles, via != 0};
        if (tuner_lds_bytes(U, D, ks, format, 1, via) <= kOnePerCu) return {1, via != 0};
    }
    return {0, false};
}

// What a call of n_wide wide samples (a multiple of D; 0: the plan alone) launches: which kernel set, the matrix kernel's tiles,
// output path and LDS, and the grid.  matrix: the shape lies in the matrix kernels' range (U <= 24, D <= 125, Tp <= 256, a window
// that fits the LDS) and the caller allows them (allow_matrix: not under tuner_variant = 1).  A matrix launch walks n_steps steps
// of 16 tiles columns (8 U outputs each) of every channel; its grid is grid_x workgroups of steps_per_wg consecutive steps each
// times grid_y rows of 16 channels: as many steps per workgroup as kTunerWorkgroups workgroups leave (the rotation table is
// loaded once per workgroup).  The generic kernel's grid is one channel times 256 outputs per workgroup; n_steps = 0 there.
// fmrx_tuner_create, tuner_launch and fmrx_tuner_plan all read this one function (tests/cpp/tuner_plan_check.cpp walks it);
// tuner_plan_of_shape is its body for a caller that holds tuner_shape(T, U, D)'s Tp and ks already.
struct TunerPlanInfo {
    bool matrix = false;
    int tiles = 0;
    bool via_lds = false;
    size_t lds_bytes = 0;
    int n_steps = 0, steps_per_wg = 0, grid_x = 0, grid_y = 0;
};
inline TunerPlanInfo tuner_plan_of_shape(int U, int D, int Tp, int ks, int format, int n_channels, long n_wide, bool allow_matrix)
{
    TunerPlanInfo p;
    const long n_out = n_wide / D * U;
    const TunerPlan plan = tuner_plan(U, D, ks, format);
    p.matrix = allow_matrix && U <= kTunerRatMfmaMaxU && D <= kTunerRatMfmaMaxD && Tp <= kTunerMfmaMaxTaps && plan.tiles > 0;
    if (!p.matrix) {
        p.grid_x = n_channels;
        p.grid_y = static_cast<int>((n_out + 255) / 256);
        return p;
    }
    p.tiles = plan.tiles;
    p.via_lds = plan.via_lds;
    p.lds_bytes = tuner_lds_bytes(U, D, ks, format, p.tiles, p.via_lds);
    const long cols = (n_out + kTunerPhases * U - 1) / (kTunerPhases * U);
    p.n_steps = static_cast<int>((cols + 16 * p.tiles - 1) / (16 * p.tiles));
    p.grid_y = (n_channels + 4 * kTunerGroup - 1) / (4 * kTunerGroup);
    p.steps_per_wg = static_cast<int>((static_cast<long>(p.n_steps) * p.grid_y + kTunerWorkgroups - 1) / kTunerWorkgroups);
    if (p.steps_per_wg < 1) p.steps_per_wg = 1;
    p.grid_x = (p.n_steps + p.steps_per_wg - 1) / p.steps_per_wg;
    return p;
}
inline TunerPlanInfo tuner_plan_info(int U, int D, int T, int format, int n_channels, long n_wide, bool allow_matrix = true)
{
    const TunerShape sh = tuner_shape(T, U, D);
    return tuner_plan_of_shape(U, D, sh.Tp, sh.ks, format, n_channels, n_wide, allow_matrix);
}
inline size_t tuner_group_image_bytes(const TunerShape &s) { return static_cast<size_t>(kTunerPhases) * s.U * s.ksp * 64 * 16; }

// One channel's rows of its group's A-operand image of v_mfma_i32_16x16x64_i8: [image q][K-step - j0[q]][lane][16 bytes],
// lane (row = lane & 15, quarter g = lane >> 4) holding what row `row` applies to window bytes 64 j + 16 g + 0..15.
// Row = 4 * (channel in group) + 2 * part + digit, part 0 = real, 1 = imaginary part of the accumulator:
//   real:  I bytes meet re[j], Q bytes meet -im[j];   imaginary:  I bytes meet im[j], Q bytes meet re[j].
// The C layout (row = 4 (lane >> 4) + register) then hands lane (column, g) channel g's four rows of one output time.
// re, im: phase-major [U * Tp], as tuner_design writes them.
inline void tuner_fill_image(int8_t *img, const TunerShape &sh, int ch_in_group, const int16_t *re, const int16_t *im)
{
    const int nq = kTunerPhases * sh.U;
    for (int q = 0; q < nq; q++) {
        const int16_t *pre = re + static_cast<size_t>(q * sh.D % sh.U) * sh.Tp, *pim = im + static_cast<size_t>(q * sh.D % sh.U) * sh.Tp;
        const int off = 2 * (q * sh.D / sh.U);
        for (int jr = 0; jr < sh.ksp; jr++)
            for (int part = 0; part < 2; part++)
                for (int d = 0; d < kTunerDigits; d++) {
                    const int row = 4 * ch_in_group + 2 * part + d;
                    for (int g = 0; g < 4; g++) {
                        int8_t *dst = img + ((static_cast<size_t>(q) * sh.ksp + jr) * 64 + (16 * g + row)) * 16;
                        for (int b = 0; b < 16; b++) {
                            const int u = 64 * (sh.j0[q] + jr) + 16 * g + b;
                            const int c = u & 1;
                            const int e = sh.front + off + c - u;            // = 2 j
                            int8_t v = 0;
                            if (e >= 0 && e / 2 <= sh.Tp - 1 && sh.j0[q] + jr < sh.j1[q]) {
                                const int k = e / 2;
                                const int t = part == 0 ? (c == 0 ? pre[k] : -pim[k]) : (c == 0 ? pim[k] : pre[k]);
                                int8_t dig[2];
                                tuner_digits(t, dig);
                                v = dig[d];
                            }
                            dst[b] = v;
                        }
                    }
                }
    }
}

}  // namespace fmrx
