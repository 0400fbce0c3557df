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
// These matrix kernels are the integer tuner's: U = 1, D = R <= 32 (the code says D), compiled for kTT / kTT16 tiles per wave.
// Every other rate U / D runs the templated ones of kernels_tuner_rational.hip.  Both sets are made of the pieces of
// tuner_mfma.hpp (wave set-up, window staging, the K-step loop tuner_mac, the epilogue tuner_finish8 / tuner_finish16); what
// the integer kernels add is the K-step ranges of the 8 phases computed once per kernel (tuner_phase_ranges), the phase word
// as a running add of w D (tuner_phase_words) and the direct store of every piece (tuner_store_piece).  tuner_launch below,
// the one entry point, sends a call to either set or to the generic kernel, and then launches tuner_hist_kernel, which carries
// the stream's last `front` values to the next call.
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
#include "tuner_mfma.hpp"

#include <type_traits>

namespace fmrx {
namespace {

constexpr int kStepOut = 128 * kTT;           // outputs per channel and step (kTT tiles per wave: tuner_host.hpp)

// K-step range of every phase, the same in every column and step (scalars)
__device__ __forceinline__ void tuner_phase_ranges(int (&j0)[kTunerPhases], int (&j1)[kTunerPhases], int D, int T, int front)
{
#pragma unroll
    for (int p = 0; p < kTunerPhases; p++) {
        j0[p] = (front + 2 * D * p - 2 * (T - 1)) / 64;
        j1[p] = (front + 2 * D * p + 1) / 64 + 1;
    }
}

// phase words of a lane's 8 outputs from output mb on: w (n0 + (mb + p) D) mod 2^32, a running add
__device__ __forceinline__ void tuner_phase_words(unsigned (&ph)[kTunerPhases], unsigned w, unsigned n0, long mb, int D)
{
    ph[0] = w * (n0 + static_cast<unsigned>(mb) * static_cast<unsigned>(D));
#pragma unroll
    for (int p = 1; p < kTunerPhases; p++) ph[p] = ph[p - 1] + w * static_cast<unsigned>(D);
}

// kFlip: as tuner_stage_bytes'
template <unsigned kFlip>
__device__ __forceinline__ void tuner_mfma_body(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int D, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    uint8_t *stage = lds_raw + kTunerTableSize * 4;
    const TunerWave tw = tuner_wave(n_channels);
    unsigned w;
    int sh;
    const i4 *a_grp = tuner_wave_setup(tw, tab, table, chan, a_img, 1, ksp, w, sh);
    int j0[kTunerPhases], j1[kTunerPhases];
    tuner_phase_ranges(j0, j1, D, T, front);
    const int n_pieces = 16 * kTT * D + 4 * ks;                     // 16-byte pieces of a step's window
    const uint8_t *const planes[1] = {stage};
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long m0 = static_cast<long>(st) * kStepOut;
        __syncthreads();                                            // the previous step's reads are done (and the table is written)
        tuner_stage_bytes<kFlip>(stage, x, hist, n_bytes, front, 2L * D * m0 - front, n_pieces, D, tw.tid);
        __syncthreads();
        if (!tw.live) continue;

        i4 acc[1][kTT][kTunerPhases];
        tuner_mac<kTT, 1>(acc, planes, a_grp, j0, j1, 0, ks, ksp, D, tw.col, tw.g);
        if (!tw.ch_ok) continue;
#pragma unroll
        for (int tt = 0; tt < kTT; tt++) {
            const long mb = m0 + 128 * tt + 8 * tw.col;             // this lane's first output time of the tile
            if (mb >= n_out) continue;
            unsigned ph[kTunerPhases], pr[kTunerPhases];
            tuner_phase_words(ph, w, n0, mb, D);
            const bool whole = mb + kTunerPhases <= n_out;
            tuner_finish8(acc[0][tt], ph, tab, sh, whole, mb, n_out, pr, clipped, power);
            tuner_store_piece(out + static_cast<long>(tw.ch) * pitch + 2 * mb, pr, whole, n_out - mb);
        }
    }
    tuner_add_levels(clipped, power, tw.ch_ok && tw.col == 0, levels + 2 * tw.ch);
}

__global__ __launch_bounds__(256, 2) void tuner_mfma_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int D, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    tuner_mfma_body<0x80u>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, D, T, front, ks, ksp, n0, n_steps, steps_per_wg, levels);
}

__global__ __launch_bounds__(256, 2) void tuner_mfma_s8_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int D, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    tuner_mfma_body<0u>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, D, T, front, ks, ksp, n0, n_steps, steps_per_wg, levels);
}

// ---- signed 16-bit input: two byte planes against the same operand image ------------------------------------------
constexpr int kStepOut16 = 128 * kTT16;       // kTT16 tiles per wave and step: two planes of accumulators each

// x, hist: raw little-endian int16 I,Q values (n_values of them in the call, `front` in the history); a plane's byte u is
// value u's low or high byte, so plane positions are the 8-bit kernel's byte positions and the raw position is twice that.
__global__ __launch_bounds__(256, 2) void tuner_mfma_s16_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_values, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const int2 *__restrict__ kconst, const unsigned *__restrict__ table, uint8_t *__restrict__ out,
    long pitch, int n_channels, long n_out, int D, int T, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    const TunerWave tw = tuner_wave(n_channels);
    const int n_pieces = 16 * kTT16 * D + 4 * ks;                   // 16-byte pieces of a step's window, per plane
    uint8_t *stage_l = lds_raw + kTunerTableSize * 4;
    uint8_t *stage_h = stage_l + tuner_plane_bytes(n_pieces, D);
    unsigned w;
    int sh;
    const i4 *a_grp = tuner_wave_setup(tw, tab, table, chan, a_img, 1, ksp, w, sh);
    int j0[kTunerPhases], j1[kTunerPhases];
    tuner_phase_ranges(j0, j1, D, T, front);
    const int2 kc = tw.ch_ok ? kconst[tw.ch] : int2{0, 0};          // U = 1: the 8 images' phase is the channel's one
    const uint8_t *const planes[2] = {stage_l, stage_h};
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long m0 = static_cast<long>(st) * kStepOut16;
        __syncthreads();
        tuner_stage_planes(stage_l, stage_h, x, hist, n_values, front, 2L * D * m0 - front, n_pieces, D, tw.tid);
        __syncthreads();
        if (!tw.live) continue;

        i4 acc[2][kTT16][kTunerPhases];                             // low plane, high plane
        tuner_mac<kTT16, 2>(acc, planes, a_grp, j0, j1, 0, ks, ksp, D, tw.col, tw.g);
        if (!tw.ch_ok) continue;
#pragma unroll
        for (int tt = 0; tt < kTT16; tt++) {
            const long mb = m0 + 128 * tt + 8 * tw.col;             // this lane's first output time of the tile
            if (mb >= n_out) continue;
            unsigned ph[kTunerPhases], pr[kTunerPhases];
            tuner_phase_words(ph, w, n0, mb, D);
            const bool whole = mb + kTunerPhases <= n_out;
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++)
                pr[p] = tuner_finish16(acc[0][tt][p], acc[1][tt][p], kc, ph[p], tab, sh, whole || mb + p < n_out, clipped, power);
            tuner_store_piece(out + static_cast<long>(tw.ch) * pitch + 2 * mb, pr, whole, n_out - mb);
        }
    }
    tuner_add_levels(clipped, power, tw.ch_ok && tw.col == 0, levels + 2 * tw.ch);
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

}  // namespace

int tuner_launch(const TunerLaunch &a, hipStream_t stream)
{
    const long n_out = a.n_bytes / 2 / a.D * a.U;
    const int vb = tuner_value_bytes(a.format);
    if (n_out > 0) {
        // which kernels, the matrix kernel's tiles, output path and LDS, and the grid: tuner_plan_info (tuner_host.hpp)
        const TunerPlanInfo plan = tuner_plan_of_shape(a.U, a.D, a.Tp, a.ks, a.format, a.n_channels, a.n_bytes / 2, a.mfma);
        if (plan.matrix) {
            const int n_steps = plan.n_steps, per = plan.steps_per_wg;
            const dim3 grid(plan.grid_x, plan.grid_y);
            const size_t lds = plan.lds_bytes;
            if (!tuner_integer_rate(a.U, a.D)) {
                FMRX_TRY(tuner_rat_mfma_launch(a, n_out, plan, stream));
            } else if (a.format == kTunerS16) {
                FMRX_TRY(tuner_launch_mfma(tuner_mfma_s16_kernel, grid, lds, stream, a.x, a.hist, a.n_bytes,
                                           reinterpret_cast<const i4 *>(a.a_img), a.chan, a.kconst, a.table, a.out, a.pitch, a.n_channels, n_out,
                                           a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, per, a.levels));
            } else {
                FMRX_TRY(tuner_launch_mfma(a.format == kTunerS8 ? tuner_mfma_s8_kernel : tuner_mfma_kernel, grid, lds, stream, a.x,
                                           a.hist, a.n_bytes, reinterpret_cast<const i4 *>(a.a_img), a.chan, a.table, a.out, a.pitch,
                                           a.n_channels, n_out, a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, per, a.levels));
            }
        } else {
            const auto kernel = a.format == kTunerS16 ? tuner_generic_s16_kernel : a.format == kTunerS8 ? tuner_generic_s8_kernel : tuner_generic_kernel;
            hipLaunchKernelGGL(kernel, dim3(plan.grid_x, plan.grid_y), dim3(256), 0, stream, a.x, a.hist,
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
