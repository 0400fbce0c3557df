// kernels_tuner.hip -- the wideband tuner's kernels and their launch: N channels' frequency-translating decimating FIRs on ONE
// wide capture (include/fmrx.h: fmrx_tuner_*; arithmetic defined by tests/_tuner_model.py).
//
//   y_c[m] = Q( e^{-j phi_c(mR)} * sum_k taps_c[k] * x[mR - k] ),   x = (u8 - 128) as complex, taps_c complex int16
//
// Everything is integer arithmetic: the complex-tap FIR on the raw bytes is exact in int32, the rotation by a 2^12-entry
// table of round(32767 cos), round(32767 sin) is exact in int64, the rounding to u8 is one add and one arithmetic shift.
//
// The matrix kernel (tuner_mfma_kernel), on v_mfma_i32_16x16x64_i8:
//   rows    (M=16) = 4 channels x {real, imaginary part of the accumulator} x 2 balanced base-256 digits of the taps
//   columns (N=16) = 16 consecutive groups of 8 output times; a column's window starts 16 R bytes after its neighbour's, a
//                    multiple of 16 for every R, so every B fragment is an aligned ds_read_b128 whatever 2 R is
//   K              = the raw interleaved bytes of a column's window (XOR 0x80 when staged); the 8 output times of a column
//                    ("phases") are 8 operand images of the same taps, shifted by 2 R bytes each, against the SAME B fragment.
// A phase's taps cover 2 T of the window's 2 T + 14 R bytes: only the K-steps its image is non-zero in are stored and
// multiplied.  Every lane holds 16 consecutive K bytes of its row / column in both operands, so the product does not depend
// on how the hardware numbers k inside a lane.
// The C layout gives lane (column, g) the four rows of channel g at one output time per phase: after the 8 phases it holds
// 8 consecutive (I, Q) byte pairs of that channel = one 16-byte piece of its output row, stored with one global_store_dwordx4
// (16 lanes: 256 contiguous bytes of a row).  No transpose, no second pass over the outputs.
// A workgroup = 4 waves = 4 channel groups (16 channels) x 512 output times per step; the step's input window (1024 R bytes
// plus the filter's reach) is staged once in LDS and shared by the four groups; the rotation table sits in LDS beside it.
// The stage is padded by 16 bytes per 16 R (the column stride) so that the 16 columns of a B read spread over the banks.
//
// These matrix kernels are the integer tuner's: U = 1, D = R <= 32, compiled for kTT / kTT16 tiles per wave.  Every other rate
// U / D runs the templated ones of kernels_tuner_rational.hip; tuner_launch below, the one entry point, sends a call to either
// or to the generic kernel, and then launches tuner_hist_kernel, which carries the stream's last `front` values to the next call.
//
// The generic kernel (tuner_generic_kernel), for every rate: one thread per (channel, output), integer loops over the Tp taps
// of the output's phase p_m = m D mod U against the samples from n_m = floor(m D / U) back (U = 1: all T taps from m R back);
// any T, U <= 32, D <= 512 -- the second device implementation the tests compare with the models (option tuner_variant = 1 /
// FMRX_TUNER_VARIANT=generic), and what runs outside the matrix kernels' range.
//
// Input formats (tuner_host.hpp; tests/_tuner_formats_model.py).  Signed 8-bit: the same two kernels without the XOR and
// with 0x00 as the zero sample (tuner_mfma_s8_kernel, tuner_generic_s8_kernel).  Signed 16-bit (tuner_mfma_s16_kernel): the
// window is staged as TWO byte planes, the low bytes (XOR 0x80: L = low byte - 128) and the high bytes (H, the int8 as it
// is), split with byte permutes while staging; each plane has exactly the layout of the 8-bit stage and meets the SAME
// operand image, into its own int32 accumulators (each within the 8-bit bound 128 sum(|re| + |im|)).  x = 256 H + L + 128,
// so acc = 256 accH + accL + 128 (row sum of the taps): the last term is a per-channel constant (TunerLaunch::kconst), the
// sum is formed in 64 bits in the epilogue, rotated and rounded as the model does with the shift s + 15 + 8.  Two tiles per
// wave and step instead of four keep the accumulators at 128 registers; every A fragment still feeds four MFMAs.
#include "fmrx_internal.hpp"
#include "tuner_host.hpp"
#include "tuner_kernels.hpp"

#include <type_traits>

namespace fmrx {
namespace {

constexpr int kTT = 4;                        // tiles (of 16 columns x 8 outputs) per wave and step
constexpr int kStepOut = 128 * kTT;           // outputs per channel and step

// kFlip: what turns a raw byte into the int8 x (0x80 for unsigned bytes, 0 for signed ones) = the raw byte of a zero sample
template <unsigned kFlip>
__device__ __forceinline__ void tuner_mfma_body(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int R, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    uint8_t *stage = lds_raw + kTunerTableSize * 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = static_cast<int>(blockIdx.y) * 4 + wave;
    const int n_groups = (n_channels + kTunerGroup - 1) / kTunerGroup;
    const bool live = grp < n_groups;                               // wave-uniform
    const int col = lane & 15, g = lane >> 4;
    const int ch = grp * kTunerGroup + g;
    const bool ch_ok = live && ch < n_channels;

    for (int i = tid; i < kTunerTableSize; i += 256) tab[i] = table[i];

    // K-step range of every phase (scalars)
    int j0[kTunerPhases], j1[kTunerPhases];
#pragma unroll
    for (int p = 0; p < kTunerPhases; p++) {
        j0[p] = (front + 2 * R * p - 2 * (T - 1)) / 64;
        j1[p] = (front + 2 * R * p + 1) / 64 + 1;
    }
    unsigned w = 0;
    int sh = 1;
    if (ch_ok) {
        const uint2 cp = chan[ch];
        w = cp.x;
        sh = static_cast<int>(cp.y);
    }
    const i4 *a_grp = a_img + static_cast<size_t>(live ? grp : 0) * kTunerPhases * ksp * 64 + lane;
    const int n_pieces = 64 * R + 4 * ks;                           // 16-byte pieces of a step's window
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long m0 = static_cast<long>(st) * kStepOut;
        const long q0 = 2L * R * m0 - front;                        // byte position of the window's start, relative to the call
        __syncthreads();                                            // the previous step's reads are done (and the table is written)
        for (int i = tid; i < n_pieces; i += 256) {
            const long q = q0 + 16L * i;
            u4 v;
            if (q < 0) {
                v = *reinterpret_cast<const u4 *>(hist + front + q);
            } else if (q + 16 <= n_bytes) {
                v = *reinterpret_cast<const u4 *>(x + q);
            } else {
                unsigned b[4];                                      // past the call: zero samples
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    unsigned wd = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const long pos = q + 4 * d + k;
                        wd |= (pos < n_bytes ? static_cast<unsigned>(x[pos]) : kFlip) << (8 * k);
                    }
                    b[d] = wd;
                }
                v = u4{b[0], b[1], b[2], b[3]};
            }
            if (kFlip) v ^= kFlip * 0x01010101u;                    // u8 -> u8 - 128 as int8
            *reinterpret_cast<u4 *>(stage + 16 * (i + i / R)) = v;
        }
        __syncthreads();
        if (!live) continue;

        i4 acc[kTT][kTunerPhases];
#pragma unroll
        for (int tt = 0; tt < kTT; tt++)
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) acc[tt][p] = i4{0, 0, 0, 0};
        // this lane's B fragment of K-step j, tile tt: piece R (16 tt + col) + 4 j + g, padded by one piece per R
        int rem = g % R, blk = g / R;                               // (4 j + g) mod R and div R
        for (int j = 0; j < ks; j++) {
            i4 b[kTT];
#pragma unroll
            for (int tt = 0; tt < kTT; tt++)
                b[tt] = *reinterpret_cast<const i4 *>(stage + 16 * ((R + 1) * (16 * tt + col) + 4 * j + g + blk));
            // the 8 phases' A fragments of this K-step, issued together (a phase outside its range loads its nearest stored step)
            i4 a[kTunerPhases];
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) {
                int jr = j - j0[p];
                jr = jr < 0 ? 0 : (jr >= ksp ? ksp - 1 : jr);
                a[p] = a_grp[(p * ksp + jr) * 64];
            }
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) {
                if (j >= j0[p] && j < j1[p]) {
#pragma unroll
                    for (int tt = 0; tt < kTT; tt++) acc[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b[tt], acc[tt][p], 0, 0, 0);
                }
            }
            rem += 4;
            while (rem >= R) {
                rem -= R;
                blk++;
            }
        }
        if (!ch_ok) continue;
#pragma unroll
        for (int tt = 0; tt < kTT; tt++) {
            const long mb = m0 + 128 * tt + 8 * col;                // this lane's first output time of the tile
            if (mb >= n_out) continue;
            unsigned pr[kTunerPhases];
            unsigned ph = w * (n0 + static_cast<unsigned>(mb) * static_cast<unsigned>(R));
            const unsigned dph = w * static_cast<unsigned>(R);
            const bool whole = mb + kTunerPhases <= n_out;
            if (sh >= 17 && sh <= 47) {
                unsigned cl[kTunerPhases], pw[kTunerPhases];
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    const int ar = acc[tt][p][0] + 256 * acc[tt][p][1], ai = acc[tt][p][2] + 256 * acc[tt][p][3];
                    cl[p] = 0;
                    pw[p] = 0;
                    pr[p] = tuner_round_pair_fast(ar, ai, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh - 16, cl[p], pw[p]);
                    ph += dph;
                }
                unsigned cs = 0, ps = 0;
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++)
                    if (whole || mb + p < n_out) {
                        cs += cl[p];
                        ps += pw[p];
                    }
                clipped += cs;
                power += ps;
            } else {
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    const int ar = acc[tt][p][0] + 256 * acc[tt][p][1], ai = acc[tt][p][2] + 256 * acc[tt][p][3];
                    unsigned cl = 0;
                    unsigned long long pw = 0;
                    pr[p] = tuner_round_pair(ar, ai, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh, cl, pw);
                    if (mb + p < n_out) {
                        clipped += cl;
                        power += pw;
                    }
                    ph += dph;
                }
            }
            tuner_store_piece(out + static_cast<long>(ch) * pitch + 2 * mb, pr, whole, n_out - mb);
        }
    }
    tuner_add_levels(clipped, power, ch_ok && col == 0, levels + 2 * ch);
}

__global__ __launch_bounds__(256, 2) void tuner_mfma_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int R, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    tuner_mfma_body<0x80u>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, R, T, front, ks, ksp, n0, n_steps, steps_per_wg, levels);
}

__global__ __launch_bounds__(256, 2) void tuner_mfma_s8_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int R, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    tuner_mfma_body<0u>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, R, T, front, ks, ksp, n0, n_steps, steps_per_wg, levels);
}

// ---- signed 16-bit input: two byte planes against the same operand image ------------------------------------------
constexpr int kTT16 = 2;                      // tiles per wave and step: two planes of accumulators each
constexpr int kStepOut16 = 128 * kTT16;

// x, hist: raw little-endian int16 I,Q values (n_values of them in the call, `front` in the history); a plane's byte u is
// value u's low or high byte, so plane positions are the 8-bit kernel's byte positions and the raw position is twice that.
__global__ __launch_bounds__(256, 2) void tuner_mfma_s16_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_values, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const int2 *__restrict__ kconst, const unsigned *__restrict__ table, uint8_t *__restrict__ out,
    long pitch, int n_channels, long n_out, int R, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = static_cast<int>(blockIdx.y) * 4 + wave;
    const int n_groups = (n_channels + kTunerGroup - 1) / kTunerGroup;
    const bool live = grp < n_groups;                               // wave-uniform
    const int col = lane & 15, g = lane >> 4;
    const int ch = grp * kTunerGroup + g;
    const bool ch_ok = live && ch < n_channels;
    const int n_pieces = 16 * kTT16 * R + 4 * ks;                   // 16-byte pieces of a step's window, per plane
    uint8_t *stage_l = lds_raw + kTunerTableSize * 4;
    uint8_t *stage_h = stage_l + 16 * (n_pieces + n_pieces / R + 1);

    for (int i = tid; i < kTunerTableSize; i += 256) tab[i] = table[i];

    int j0[kTunerPhases], j1[kTunerPhases];
#pragma unroll
    for (int p = 0; p < kTunerPhases; p++) {
        j0[p] = (front + 2 * R * p - 2 * (T - 1)) / 64;
        j1[p] = (front + 2 * R * p + 1) / 64 + 1;
    }
    unsigned w = 0;
    int sh = 1, kr = 0, ki = 0;
    if (ch_ok) {
        const uint2 cp = chan[ch];
        w = cp.x;
        sh = static_cast<int>(cp.y);
        const int2 kc = kconst[ch];
        kr = kc.x;
        ki = kc.y;
    }
    const i4 *a_grp = a_img + static_cast<size_t>(live ? grp : 0) * kTunerPhases * ksp * 64 + lane;
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long m0 = static_cast<long>(st) * kStepOut16;
        const long q0 = 2L * R * m0 - front;                        // plane position of the window's start, relative to the call
        __syncthreads();
        for (int i = tid; i < n_pieces; i += 256) {
            const long q = q0 + 16L * i;
            u4 v0, v1;                                              // 16 values = 32 raw bytes -> one piece per plane
            if (q < 0) {
                const u4 *src = reinterpret_cast<const u4 *>(hist + 2 * (front + q));
                v0 = src[0];
                v1 = src[1];
            } else if (q + 16 <= n_values) {
                const u4 *src = reinterpret_cast<const u4 *>(x + 2 * q);
                v0 = src[0];
                v1 = src[1];
            } else {
                unsigned b[8];                                      // past the call: zero samples
#pragma unroll
                for (int d = 0; d < 8; d++) {
                    unsigned wd = 0;
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const long pos = q + 2 * d + k;
                        wd |= (pos < n_values ? static_cast<unsigned>(reinterpret_cast<const unsigned short *>(x)[pos]) : 0u) << (16 * k);
                    }
                    b[d] = wd;
                }
                v0 = u4{b[0], b[1], b[2], b[3]};
                v1 = u4{b[4], b[5], b[6], b[7]};
            }
            // a raw word is (low, high) of value 2 d, (low, high) of value 2 d + 1: even bytes -> low plane, odd -> high plane
            const u4 lo = u4{__builtin_amdgcn_perm(v0[1], v0[0], 0x06040200u), __builtin_amdgcn_perm(v0[3], v0[2], 0x06040200u),
                             __builtin_amdgcn_perm(v1[1], v1[0], 0x06040200u), __builtin_amdgcn_perm(v1[3], v1[2], 0x06040200u)};
            const u4 hi = u4{__builtin_amdgcn_perm(v0[1], v0[0], 0x07050301u), __builtin_amdgcn_perm(v0[3], v0[2], 0x07050301u),
                             __builtin_amdgcn_perm(v1[1], v1[0], 0x07050301u), __builtin_amdgcn_perm(v1[3], v1[2], 0x07050301u)};
            const int off = 16 * (i + i / R);
            *reinterpret_cast<u4 *>(stage_l + off) = lo ^ 0x80808080u;   // low byte - 128 as int8
            *reinterpret_cast<u4 *>(stage_h + off) = hi;
        }
        __syncthreads();
        if (!live) continue;

        i4 accl[kTT16][kTunerPhases], acch[kTT16][kTunerPhases];
#pragma unroll
        for (int tt = 0; tt < kTT16; tt++)
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) accl[tt][p] = acch[tt][p] = i4{0, 0, 0, 0};
        int rem = g % R, blk = g / R;                               // (4 j + g) mod R and div R
        for (int j = 0; j < ks; j++) {
            i4 bl[kTT16], bh[kTT16];
#pragma unroll
            for (int tt = 0; tt < kTT16; tt++) {
                const int off = 16 * ((R + 1) * (16 * tt + col) + 4 * j + g + blk);
                bl[tt] = *reinterpret_cast<const i4 *>(stage_l + off);
                bh[tt] = *reinterpret_cast<const i4 *>(stage_h + off);
            }
            i4 a[kTunerPhases];
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) {
                int jr = j - j0[p];
                jr = jr < 0 ? 0 : (jr >= ksp ? ksp - 1 : jr);
                a[p] = a_grp[(p * ksp + jr) * 64];
            }
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) {
                if (j >= j0[p] && j < j1[p]) {
#pragma unroll
                    for (int tt = 0; tt < kTT16; tt++) {
                        accl[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], bl[tt], accl[tt][p], 0, 0, 0);
                        acch[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], bh[tt], acch[tt][p], 0, 0, 0);
                    }
                }
            }
            rem += 4;
            while (rem >= R) {
                rem -= R;
                blk++;
            }
        }
        if (!ch_ok) continue;
#pragma unroll
        for (int tt = 0; tt < kTT16; tt++) {
            const long mb = m0 + 128 * tt + 8 * col;                // this lane's first output time of the tile
            if (mb >= n_out) continue;
            unsigned pr[kTunerPhases];
            unsigned ph = w * (n0 + static_cast<unsigned>(mb) * static_cast<unsigned>(R));
            const unsigned dph = w * static_cast<unsigned>(R);
            const bool whole = mb + kTunerPhases <= n_out;
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) {
                const int lr = accl[tt][p][0] + 256 * accl[tt][p][1], li = accl[tt][p][2] + 256 * accl[tt][p][3];
                const int hr = acch[tt][p][0] + 256 * acch[tt][p][1], hi = acch[tt][p][2] + 256 * acch[tt][p][3];
                unsigned cl = 0;
                unsigned long long pw = 0;
                pr[p] = tuner_round_pair_planes(lr, li, hr, hi, kr, ki, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh, cl, pw);
                if (whole || mb + p < n_out) {
                    clipped += cl;
                    power += pw;
                }
                ph += dph;
            }
            tuner_store_piece(out + static_cast<long>(ch) * pitch + 2 * mb, pr, whole, n_out - mb);
        }
    }
    tuner_add_levels(clipped, power, ch_ok && col == 0, levels + 2 * ch);
}

// FMT: kTunerU8 / kTunerS8 / kTunerS16.  x, hist: raw values (bytes, or little-endian int16 for S16); the 16-bit format's sums
// need 64 bits (|acc| < 2^40), the 8-bit formats' fit int32.  taps_re, taps_im: [n_channels][U * Tp] phase-major.
template <int FMT>
__device__ __forceinline__ void tuner_generic_body(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, const int16_t *__restrict__ taps_re,
    const int16_t *__restrict__ taps_im, const uint2 *__restrict__ chan, const unsigned *__restrict__ table,
    uint8_t *__restrict__ out, long pitch, long n_out, int U, int D, int Tp, int front, unsigned n0, unsigned long long *__restrict__ levels)
{
    using value_t = std::conditional_t<FMT == kTunerS16, int16_t, std::conditional_t<FMT == kTunerS8, int8_t, uint8_t>>;
    using acc_t = std::conditional_t<FMT == kTunerS16, long long, int>;
    constexpr int kBias = FMT == kTunerU8 ? 128 : 0;
    const value_t *xv = reinterpret_cast<const value_t *>(x), *hv = reinterpret_cast<const value_t *>(hist);
    const int ch = blockIdx.x;
    const long m = static_cast<long>(blockIdx.y) * 256 + threadIdx.x;
    unsigned clipped = 0;
    unsigned long long power = 0;
    if (m < n_out) {
        long nm = m * D;                                            // the output's newest sample and its phase
        int p = 0;
        if (U != 1) {                                               // wave-uniform: the integer tuner skips the 64-bit division
            const long md = nm;
            nm = md / U;
            p = static_cast<int>(md - nm * U);
        }
        const int16_t *re = taps_re + (static_cast<long>(ch) * U + p) * Tp, *im = taps_im + (static_cast<long>(ch) * U + p) * Tp;
        acc_t ar = 0, ai = 0;
        for (int j = 0; j < Tp; j++) {
            const long pos = 2 * (nm - j);
            const value_t *src = pos < 0 ? hv + front + pos : xv + pos;
            const int xr = static_cast<int>(src[0]) - kBias, xq = static_cast<int>(src[1]) - kBias;
            const int gr = re[j], gi = im[j];
            ar += static_cast<acc_t>(gr * xr) - gi * xq;            // a product is below 2^30, a difference of two is not
            ai += static_cast<acc_t>(gi * xr) + gr * xq;
        }
        const uint2 cp = chan[ch];
        const unsigned ph = cp.x * (n0 + static_cast<unsigned>(nm));
        const Rot r = rot_of(table[ph >> (32 - kTunerTableBits)]);
        const long long yr = static_cast<long long>(ar) * r.c + static_cast<long long>(ai) * r.s;
        const long long yi = static_cast<long long>(ai) * r.c - static_cast<long long>(ar) * r.s;
        const unsigned pr = tuner_round_y(yr, yi, static_cast<int>(cp.y), clipped, power);
        *reinterpret_cast<unsigned short *>(out + static_cast<long>(ch) * pitch + 2 * m) = static_cast<unsigned short>(pr);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        clipped += __shfl_xor(clipped, o);
        power += __shfl_xor(power, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (clipped) atomicAdd(levels + 2 * ch, static_cast<unsigned long long>(clipped));
        if (power) atomicAdd(levels + 2 * ch + 1, power);
    }
}

#define FMRX_TUNER_GENERIC(NAME, FMT)                                                                                                    \
    __global__ __launch_bounds__(256) void NAME(                                                                                             \
        const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, const int16_t *__restrict__ taps_re,                                \
        const int16_t *__restrict__ taps_im, const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, \
        long pitch, long n_out, int U, int D, int Tp, int front, unsigned n0, unsigned long long *__restrict__ levels)                       \
    {                                                                                                                                        \
        tuner_generic_body<FMT>(x, hist, taps_re, taps_im, chan, table, out, pitch, n_out, U, D, Tp, front, n0, levels);                 \
    }
FMRX_TUNER_GENERIC(tuner_generic_kernel, kTunerU8)
FMRX_TUNER_GENERIC(tuner_generic_s8_kernel, kTunerS8)
FMRX_TUNER_GENERIC(tuner_generic_s16_kernel, kTunerS16)
#undef FMRX_TUNER_GENERIC

// the carried history: the last `front` raw bytes of (old history | this call's input)
__global__ __launch_bounds__(256) void tuner_hist_kernel(const uint8_t *__restrict__ x, long n_bytes, const uint8_t *__restrict__ old_hist,
                                                         uint8_t *__restrict__ new_hist, int front)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= front) return;
    const long pos = n_bytes - front + i;
    new_hist[i] = pos < 0 ? old_hist[front + pos] : x[pos];
}

constexpr size_t kTwoPerCu = 64 * 1024, kOnePerCu = 160 * 1024;     // LDS of a workgroup: two on a CU, or one

}  // namespace

// Tiles per wave and step, and whether the outputs go through the LDS buffer.  The integer kernels are compiled for kTT / kTT16
// tiles and store directly.  The rational ones, in order of preference: the buffer with the most tiles that keep two workgroups
// on a CU; the buffer with one tile and one workgroup per CU; direct stores, by the same two rules.  tiles = 0: the window does
// not fit the matrix kernel at all.
TunerPlan tuner_plan(int U, int D, int ks, int format)
{
    if (tuner_integer_rate(U, D)) return {format == kTunerS16 ? kTT16 : kTT, false};
    for (int via = 1; via >= 0; via--) {
        for (int tiles = format == kTunerS16 ? 2 : 4; tiles >= 1; tiles >>= 1)
            if (tuner_lds_bytes(U, D, ks, format, tiles, via) <= kTwoPerCu) return {tiles, via != 0};
        if (tuner_lds_bytes(U, D, ks, format, 1, via) <= kOnePerCu) return {1, via != 0};
    }
    return {0, false};
}

int tuner_launch(const TunerLaunch &a, hipStream_t stream)
{
    const long n_out = a.n_bytes / 2 / a.D * a.U;
    const int vb = tuner_value_bytes(a.format);
    if (n_out > 0) {
        if (a.mfma) {
            const long cols = (n_out + kTunerPhases * a.U - 1) / (kTunerPhases * a.U);
            const int n_steps = static_cast<int>((cols + 16 * a.tiles - 1) / (16 * a.tiles));
            const int gy = (a.n_channels + 4 * kTunerGroup - 1) / (4 * kTunerGroup);
            // enough workgroups to fill the chip a few times over, as many steps each as that leaves (the table is loaded once
            // per workgroup)
            int per = static_cast<int>((static_cast<long>(n_steps) * gy + 2047) / 2048);
            if (per < 1) per = 1;
            const int gx = (n_steps + per - 1) / per;
            const size_t lds = tuner_lds_bytes(a.U, a.D, a.ks, a.format, a.tiles, a.via_lds);
            if (!tuner_integer_rate(a.U, a.D)) {
                FMRX_TRY(tuner_rat_mfma_launch(a, n_out, n_steps, per, dim3(gx, gy), lds, stream));
            } else if (a.format == kTunerS16) {
                hipLaunchKernelGGL(tuner_mfma_s16_kernel, dim3(gx, gy), dim3(256), lds, stream, a.x, a.hist, a.n_bytes,
                                   reinterpret_cast<const i4 *>(a.a_img), a.chan, a.kconst, a.table, a.out, a.pitch, a.n_channels, n_out, a.D,
                                   a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, per, a.levels);
            } else {
                hipLaunchKernelGGL(a.format == kTunerS8 ? tuner_mfma_s8_kernel : tuner_mfma_kernel, dim3(gx, gy), dim3(256), lds, stream, a.x,
                                   a.hist, a.n_bytes, reinterpret_cast<const i4 *>(a.a_img), a.chan, a.table, a.out, a.pitch, a.n_channels,
                                   n_out, a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, per, a.levels);
            }
        } else {
            const auto kernel = a.format == kTunerS16 ? tuner_generic_s16_kernel : a.format == kTunerS8 ? tuner_generic_s8_kernel : tuner_generic_kernel;
            hipLaunchKernelGGL(kernel, dim3(a.n_channels, static_cast<unsigned>((n_out + 255) / 256)), dim3(256), 0, stream, a.x, a.hist,
                               a.taps_re, a.taps_im, a.chan, a.table, a.out, a.pitch, n_out, a.U, a.D, a.Tp, a.front, a.n0, a.levels);
        }
        FMRX_LAUNCH_CHECK("tuner_%s_kernel (format %d, %d/%d)", a.mfma ? "mfma" : "generic", a.format, a.U, a.D);
    }
    const int front_bytes = a.front * vb;
    hipLaunchKernelGGL(tuner_hist_kernel, dim3((front_bytes + 255) / 256), dim3(256), 0, stream, a.x, a.n_bytes * vb, a.hist, a.hist_next,
                       front_bytes);
    FMRX_LAUNCH_CHECK("tuner_hist_kernel");
    return FMRX_OK;
}

}  // namespace fmrx
