// kernels_tuner_rational.hip -- the wideband tuner's matrix kernels at a rational rate rf_Fs = Fs_w * U / D: N channels'
// polyphase frequency-translating FIRs on ONE wide capture (include/fmrx.h: fmrx_tuner_create_rational; DESIGN.md section 4.9.2;
// arithmetic defined by tests/_tuner_rational_model.py).  For output m of the stream, n_m = floor(m D / U), p_m = m D mod U:
//
//   y_c[m] = Q( e^{-j phi_c(n_m)} * sum_{j<Tp} taps_c[p_m][j] * x[n_m - j] ),   taps_c complex int16, phase-major [U][Tp]
//
// Integer arithmetic throughout, as in kernels_tuner.hip.  The kernels here are made of the same pieces as the integer tuner's
// (tuner_mfma.hpp: wave set-up, window staging, the K-step loop tuner_mac, the epilogue tuner_finish8 / tuner_finish16; rounding
// and stores in tuner_kernels.hpp).  What this file adds: the TT template, the loop over the U blocks of a column with
// rat_block(u)'s K-step ranges and sample offsets, the phase word w (n_b + nq[p]) and the constant of each image's phase, and
// the output path rat_emit / rat_flush / rat_wave_sync.
//
// The matrix kernels (tuner_rat_mfma_kernel, _s8_, _s16_), on v_mfma_i32_16x16x64_i8:
//   rows    (M=16) = 4 channels x {real, imaginary part of the accumulator} x 2 balanced base-256 digits of the taps
//   columns (N=16) = 16 consecutive groups of 8 U output times; a column's window starts 16 D bytes (8 D wide samples, a
//                    whole number of periods) after its neighbour's: a multiple of 16 for every D, so every B fragment
//                    is an aligned ds_read_b128
//   K              = the raw interleaved bytes of a column's window; the 8 U output times of a column are 8 U operand images
//                    against the SAME B fragments, image q holding the taps of phase q D mod U shifted by 2 floor(q D / U)
//                    bytes.  Only the K-steps an image is non-zero in are stored and multiplied.
// Every lane holds 16 consecutive K bytes of its row / column in both operands, so the product does not depend on how the
// hardware numbers k inside a lane.
// A column is walked in U blocks of 8 output times: block u (images 8 u .. 8 u + 7) makes its own pass over the K-steps it
// needs, reading B from LDS again, and ends in the integer kernel's epilogue: lane (column, g) holds 8 consecutive (I, Q)
// pairs of channel g starting at output (column index) 8 U + 8 u = one 16-byte piece.  Stored straight from there, a wave's 16
// lanes would write pieces 16 U bytes apart and the U blocks of the step would fill the gaps one pass of the K-steps later
// each: measured, that doubles the bytes written to memory (profiles/tuner_rational).  So the pieces of a step go to a
// per-wave LDS buffer laid out as the rows are (tile, channel: 16 columns x 16 U bytes = 256 U contiguous bytes of a row),
// and after the step's last block the wave writes each row segment with whole-wave contiguous 16-byte stores (rat_flush).
// Where that buffer (4 waves x TT x U KiB) does not fit the LDS beside the window, the pieces are stored directly.
// A workgroup = 4 waves = 4 channel groups x TT tiles per step; TT (4, 2 or 1) is the largest whose staged window, 256 D bytes
// per tile plus the reach, keeps two workgroups on a CU.  The 16-bit kernel stages two byte planes (tuner_stage_planes); its
// constant 128 (row sum of the taps) is a pair per PHASE, U pairs per channel.
//
// Launched by tuner_launch (kernels_tuner.hip) through tuner_rat_mfma_launch for every rate outside the integer tuner's
// (U = 1, D <= 32), with the tiles and the output path of tuner_plan_info (tuner_host.hpp).  The generic kernels and the history kernel, one set
// for all rates, are in kernels_tuner.hip.
#include "fmrx_internal.hpp"
#include "tuner_host.hpp"
#include "tuner_mfma.hpp"

namespace fmrx {
namespace {

// K-step range of the 8 images of block u, and the images' sample offsets floor(q D / U) (wave-uniform scalars)
struct RatBlock {
    int j0[kTunerPhases], j1[kTunerPhases], nq[kTunerPhases];
};
__device__ __forceinline__ RatBlock rat_block(int u, int U, int D, int Tp, int front)
{
    RatBlock b;
#pragma unroll
    for (int p = 0; p < kTunerPhases; p++) {
        const int q = kTunerPhases * u + p;
        b.nq[p] = q * D / U;
        b.j0[p] = (front + 2 * b.nq[p] - 2 * (Tp - 1)) / 64;
        b.j1[p] = (front + 2 * b.nq[p] + 1) / 64 + 1;
    }
    return b;
}

// A step's outputs of one wave, from its LDS buffer to the rows: segment (tile tt, channel g of the group) = 256 U contiguous
// bytes starting at byte (c0 + 16 tt) 16 U of the channel's row; 64 lanes store 1 KiB of it per instruction.  Bytes past the
// call's end (2 n_out, a multiple of 2 U but not of 16) are not written.
__device__ __forceinline__ void rat_flush(const uint8_t *obuf, uint8_t *__restrict__ out, long pitch, int grp, int n_channels, long c0,
                                          long n_out, int U, int tiles, int lane)
{
    const int seg_bytes = 256 * U;
    for (int seg = 0; seg < 4 * tiles; seg++) {
        const int tt = seg >> 2, ch = grp * kTunerGroup + (seg & 3);
        const long b0 = (c0 + 16 * tt) * 16L * U;
        long valid = 2 * n_out - b0;
        if (ch >= n_channels || valid <= 0) continue;               // wave-uniform
        if (valid > seg_bytes) valid = seg_bytes;
        uint8_t *dst = out + static_cast<long>(ch) * pitch + b0;
        const uint8_t *src = obuf + seg * seg_bytes;
        for (int b = 16 * lane; b < valid; b += 16 * 64) {
            const u4 v = *reinterpret_cast<const u4 *>(src + b);
            if (b + 16 <= valid) {
                *reinterpret_cast<u4 *>(dst + b) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (b + 2 * k < valid) *reinterpret_cast<unsigned short *>(dst + b + 2 * k) = static_cast<unsigned short>(v[k >> 1] >> (16 * (k & 1)));
            }
        }
    }
}

// a lane's piece of block u: to the wave's LDS buffer (row layout, see rat_flush) or straight to the row
__device__ __forceinline__ void rat_emit(uint8_t *obuf, bool via_lds, int tt, int g, int col, int u, int U, uint8_t *dst,
                                         const unsigned (&pr)[kTunerPhases], bool whole, long n_left)
{
    if (via_lds)
        *reinterpret_cast<u4 *>(obuf + (((tt * 4 + g) * 16 + col) * U + u) * 16) =
            u4{pr[0] | (pr[1] << 16), pr[2] | (pr[3] << 16), pr[4] | (pr[5] << 16), pr[6] | (pr[7] << 16)};
    else
        tuner_store_piece(dst, pr, whole, n_left);
}

// the wave's own stores to its LDS buffer are visible to all its lanes
__device__ __forceinline__ void rat_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The phase words of block u's 8 outputs in column cidx: the images' newest samples are nq[p] samples into the column
__device__ __forceinline__ void rat_phase_words(unsigned (&ph)[kTunerPhases], unsigned w, unsigned n0, long cidx, int D, const RatBlock &rb)
{
    const unsigned nb = n0 + static_cast<unsigned>(cidx) * static_cast<unsigned>(kTunerPhases * D);
#pragma unroll
    for (int p = 0; p < kTunerPhases; p++) ph[p] = w * (nb + static_cast<unsigned>(rb.nq[p]));
}

// kFlip: as tuner_stage_bytes';  TT: tiles (of 16 columns x 8 U outputs) per wave and step
template <unsigned kFlip, int TT>
__device__ __forceinline__ void tuner_rat_mfma_body(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,
    long n_out, int U, int D, int Tp, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg, int via_lds,
    unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    uint8_t *stage = lds_raw + kTunerTableSize * 4;
    const TunerWave tw = tuner_wave(n_channels);
    unsigned w;
    int sh;
    const i4 *a_grp = tuner_wave_setup(tw, tab, table, chan, a_img, U, ksp, w, sh);
    const int n_pieces = 16 * TT * D + 4 * ks;                      // 16-byte pieces of a step's window
    uint8_t *obuf = stage + tuner_plane_bytes(n_pieces, D) + tw.wave * (TT * 4 * 256 * U);   // this wave's output buffer (via_lds)
    const uint8_t *const planes[1] = {stage};
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long c0 = static_cast<long>(st) * (16 * TT);          // the step's first column
        __syncthreads();                                            // the previous step's reads are done (and the table is written)
        tuner_stage_bytes<kFlip>(stage, x, hist, n_bytes, front, 16L * D * c0 - front, n_pieces, D, tw.tid);
        __syncthreads();
        if (!tw.live) continue;

        for (int u = 0; u < U; u++) {
            const RatBlock rb = rat_block(u, U, D, Tp, front);
            i4 acc[1][TT][kTunerPhases];
            tuner_mac<TT, 1>(acc, planes, a_grp + kTunerPhases * u * ksp * 64, rb.j0, rb.j1, rb.j0[0], rb.j1[kTunerPhases - 1], ksp, D, tw.col, tw.g);
            if (tw.ch_ok) {
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const long cidx = c0 + 16 * tt + tw.col;        // this lane's column of the call
                    const long mb = (cidx * U + u) * kTunerPhases;  // its first output time of the block
                    if (mb >= n_out) continue;
                    unsigned ph[kTunerPhases], pr[kTunerPhases];
                    rat_phase_words(ph, w, n0, cidx, D, rb);
                    const bool whole = mb + kTunerPhases <= n_out;
                    tuner_finish8(acc[0][tt], ph, tab, sh, whole, mb, n_out, pr, clipped, power);
                    rat_emit(obuf, via_lds, tt, tw.g, tw.col, u, U, out + static_cast<long>(tw.ch) * pitch + 2 * mb, pr, whole, n_out - mb);
                }
            }
        }
        if (via_lds) {
            rat_wave_sync();
            rat_flush(obuf, out, pitch, tw.grp, n_channels, c0, n_out, U, TT, tw.lane);
            rat_wave_sync();
        }
    }
    tuner_add_levels(clipped, power, tw.ch_ok && tw.col == 0, levels + 2 * tw.ch);
}

#define FMRX_TUNER_RAT_ARGS                                                                                                             \
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes, const i4 *__restrict__ a_img,                        \
        const uint2 *__restrict__ chan, const unsigned *__restrict__ table, uint8_t *__restrict__ out, long pitch, int n_channels,      \
        long n_out, int U, int D, int Tp, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg, int via_lds,          \
        unsigned long long *__restrict__ levels

template <int TT>
__global__ __launch_bounds__(256, 2) void tuner_rat_mfma_kernel(FMRX_TUNER_RAT_ARGS)
{
    tuner_rat_mfma_body<0x80u, TT>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, U, D, Tp, front, ks, ksp, n0, n_steps,
                                   steps_per_wg, via_lds, levels);
}

template <int TT>
__global__ __launch_bounds__(256, 2) void tuner_rat_mfma_s8_kernel(FMRX_TUNER_RAT_ARGS)
{
    tuner_rat_mfma_body<0u, TT>(x, hist, n_bytes, a_img, chan, table, out, pitch, n_channels, n_out, U, D, Tp, front, ks, ksp, n0, n_steps,
                                steps_per_wg, via_lds, levels);
}
#undef FMRX_TUNER_RAT_ARGS

// ---- signed 16-bit input: two byte planes against the same operand image ------------------------------------------
// x, hist: raw little-endian int16 I,Q values (n_values of them in the call, `front` in the history); plane positions are
// the 8-bit kernel's byte positions, the raw position is twice that.  kconst: [n_channels][U] = 128 * {sum(re - im),
// sum(im + re)} of each phase's taps.
template <int TT>
__global__ __launch_bounds__(256, 2) void tuner_rat_mfma_s16_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_values, const i4 *__restrict__ a_img,
    const uint2 *__restrict__ chan, const int2 *__restrict__ kconst, const unsigned *__restrict__ table, uint8_t *__restrict__ out,
    long pitch, int n_channels, long n_out, int U, int D, int Tp, int front, int ks, int ksp, unsigned n0, int n_steps, int steps_per_wg,
    int via_lds, unsigned long long *__restrict__ levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    unsigned *tab = reinterpret_cast<unsigned *>(lds_raw);
    const TunerWave tw = tuner_wave(n_channels);
    const int n_pieces = 16 * TT * D + 4 * ks;                      // 16-byte pieces of a step's window, per plane
    uint8_t *stage_l = lds_raw + kTunerTableSize * 4;
    uint8_t *stage_h = stage_l + tuner_plane_bytes(n_pieces, D);
    uint8_t *obuf = stage_h + tuner_plane_bytes(n_pieces, D) + tw.wave * (TT * 4 * 256 * U);   // this wave's output buffer (via_lds)
    unsigned w;
    int sh;
    const i4 *a_grp = tuner_wave_setup(tw, tab, table, chan, a_img, U, ksp, w, sh);
    const int2 *kc_ch = kconst + static_cast<size_t>(tw.ch_ok ? tw.ch : 0) * U;
    const uint8_t *const planes[2] = {stage_l, stage_h};
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long c0 = static_cast<long>(st) * (16 * TT);
        __syncthreads();
        tuner_stage_planes(stage_l, stage_h, x, hist, n_values, front, 16L * D * c0 - front, n_pieces, D, tw.tid);
        __syncthreads();
        if (!tw.live) continue;

        for (int u = 0; u < U; u++) {
            const RatBlock rb = rat_block(u, U, D, Tp, front);
            i4 acc[2][TT][kTunerPhases];                            // low plane, high plane
            tuner_mac<TT, 2>(acc, planes, a_grp + kTunerPhases * u * ksp * 64, rb.j0, rb.j1, rb.j0[0], rb.j1[kTunerPhases - 1], ksp, D, tw.col, tw.g);
            if (tw.ch_ok) {
                int2 kc[kTunerPhases];                              // the constants of the 8 images' phases
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) kc[p] = kc_ch[(kTunerPhases * u + p) * D % U];
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const long cidx = c0 + 16 * tt + tw.col;
                    const long mb = (cidx * U + u) * kTunerPhases;
                    if (mb >= n_out) continue;
                    unsigned ph[kTunerPhases], pr[kTunerPhases];
                    rat_phase_words(ph, w, n0, cidx, D, rb);
                    const bool whole = mb + kTunerPhases <= n_out;
#pragma unroll
                    for (int p = 0; p < kTunerPhases; p++)
                        pr[p] = tuner_finish16(acc[0][tt][p], acc[1][tt][p], kc[p], ph[p], tab, sh, whole || mb + p < n_out, clipped, power);
                    rat_emit(obuf, via_lds, tt, tw.g, tw.col, u, U, out + static_cast<long>(tw.ch) * pitch + 2 * mb, pr, whole, n_out - mb);
                }
            }
        }
        if (via_lds) {
            rat_wave_sync();
            rat_flush(obuf, out, pitch, tw.grp, n_channels, c0, n_out, U, TT, tw.lane);
            rat_wave_sync();
        }
    }
    tuner_add_levels(clipped, power, tw.ch_ok && tw.col == 0, levels + 2 * tw.ch);
}

}  // namespace

int tuner_rat_mfma_launch(const TunerLaunch &a, long n_out, const TunerPlanInfo &plan, hipStream_t stream)
{
    const i4 *img = reinterpret_cast<const i4 *>(a.a_img);
    const int via = plan.via_lds, tiles = plan.tiles, n_steps = plan.n_steps, steps_per_wg = plan.steps_per_wg;
    const dim3 grid(plan.grid_x, plan.grid_y);
    const size_t lds = plan.lds_bytes;
    if (a.format == kTunerS16) {
        const auto kernel = tiles == 2 ? tuner_rat_mfma_s16_kernel<2> : tuner_rat_mfma_s16_kernel<1>;
        return tuner_launch_mfma(kernel, grid, lds, stream, a.x, a.hist, a.n_bytes, img, a.chan, a.kconst, a.table, a.out, a.pitch, a.n_channels,
                                 n_out, a.U, a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, steps_per_wg, via, a.levels);
    }
    const auto kernel = a.format == kTunerS8
                            ? (tiles == 4 ? tuner_rat_mfma_s8_kernel<4> : tiles == 2 ? tuner_rat_mfma_s8_kernel<2> : tuner_rat_mfma_s8_kernel<1>)
                            : (tiles == 4 ? tuner_rat_mfma_kernel<4> : tiles == 2 ? tuner_rat_mfma_kernel<2> : tuner_rat_mfma_kernel<1>);
    return tuner_launch_mfma(kernel, grid, lds, stream, a.x, a.hist, a.n_bytes, img, a.chan, a.table, a.out, a.pitch, a.n_channels, n_out, a.U,
                             a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, steps_per_wg, via, a.levels);
}

}  // namespace fmrx
