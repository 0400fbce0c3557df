// kernels_tuner_rational.hip -- the wideband tuner's matrix kernels at a rational rate rf_Fs = Fs_w * U / D: N channels'
// polyphase frequency-translating FIRs on ONE wide capture (include/fmrx.h: fmrx_tuner_create_rational; DESIGN.md section 4.9.2;
// arithmetic defined by tests/_tuner_rational_model.py).  For output m of the stream, n_m = floor(m D / U), p_m = m D mod U:
//
//   y_c[m] = Q( e^{-j phi_c(n_m)} * sum_{j<Tp} taps_c[p_m][j] * x[n_m - j] ),   taps_c complex int16, phase-major [U][Tp]
//
// Integer arithmetic throughout, as in kernels_tuner.hip, whose device helpers (tuner_kernels.hpp) round and store here too.
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
// per tile plus the reach, keeps two workgroups on a CU.  The 16-bit kernel stages two byte planes as tuner_mfma_s16_kernel
// does; its constant 128 (row sum of the taps) is a pair per PHASE, U pairs per channel.
//
// Launched by tuner_launch (kernels_tuner.hip) through tuner_rat_mfma_launch for every rate outside the integer tuner's
// (U = 1, D <= 32), with the tiles and the output path tuner_plan chose.  The generic kernels and the history kernel, one set
// for all rates, are in kernels_tuner.hip.
#include "fmrx_internal.hpp"
#include "tuner_host.hpp"
#include "tuner_kernels.hpp"

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

// kFlip: what turns a raw byte into the int8 x (0x80 for unsigned bytes, 0 for signed ones) = the raw byte of a zero sample
// TT: tiles (of 16 columns x 8 U outputs) per wave and step
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
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = static_cast<int>(blockIdx.y) * 4 + wave;
    const int n_groups = (n_channels + kTunerGroup - 1) / kTunerGroup;
    const bool live = grp < n_groups;                               // wave-uniform
    const int col = lane & 15, g = lane >> 4;
    const int ch = grp * kTunerGroup + g;
    const bool ch_ok = live && ch < n_channels;

    for (int i = tid; i < kTunerTableSize; i += 256) tab[i] = table[i];

    unsigned w = 0;
    int sh = 1;
    if (ch_ok) {
        const uint2 cp = chan[ch];
        w = cp.x;
        sh = static_cast<int>(cp.y);
    }
    const i4 *a_grp = a_img + static_cast<size_t>(live ? grp : 0) * kTunerPhases * U * ksp * 64 + lane;
    const int n_pieces = 16 * TT * D + 4 * ks;                      // 16-byte pieces of a step's window
    uint8_t *obuf = stage + 16 * (n_pieces + n_pieces / D + 1) + wave * (TT * 4 * 256 * U);   // this wave's output buffer (via_lds)
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long c0 = static_cast<long>(st) * (16 * TT);          // the step's first column
        const long q0 = 16L * D * c0 - front;                       // byte position of the window's start, relative to the call
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
            *reinterpret_cast<u4 *>(stage + 16 * (i + i / D)) = v;
        }
        __syncthreads();
        if (!live) continue;

        for (int u = 0; u < U; u++) {
            const RatBlock rb = rat_block(u, U, D, Tp, front);
            i4 acc[TT][kTunerPhases];
#pragma unroll
            for (int tt = 0; tt < TT; tt++)
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) acc[tt][p] = i4{0, 0, 0, 0};
            // this lane's B fragment of K-step j, tile tt: piece D (16 tt + col) + 4 j + g, padded by one piece per D
            const int jlo = rb.j0[0], jhi = rb.j1[kTunerPhases - 1];
            int rem = (4 * jlo + g) % D, blk = (4 * jlo + g) / D;   // (4 j + g) mod D and div D
            for (int j = jlo; j < jhi; j++) {
                i4 b[TT];
#pragma unroll
                for (int tt = 0; tt < TT; tt++)
                    b[tt] = *reinterpret_cast<const i4 *>(stage + 16 * ((D + 1) * (16 * tt + col) + 4 * j + g + blk));
                // the 8 images' A fragments of this K-step (an image outside its range loads its nearest stored step)
                i4 a[kTunerPhases];
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    int jr = j - rb.j0[p];
                    jr = jr < 0 ? 0 : (jr >= ksp ? ksp - 1 : jr);
                    a[p] = a_grp[((kTunerPhases * u + p) * ksp + jr) * 64];
                }
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    if (j >= rb.j0[p] && j < rb.j1[p]) {
#pragma unroll
                        for (int tt = 0; tt < TT; tt++) acc[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b[tt], acc[tt][p], 0, 0, 0);
                    }
                }
                rem += 4;
                while (rem >= D) {
                    rem -= D;
                    blk++;
                }
            }
            if (ch_ok) {
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const long cidx = c0 + 16 * tt + col;           // this lane's column of the call
                    const long mb = (cidx * U + u) * kTunerPhases;  // its first output time of the block
                    if (mb >= n_out) continue;
                    unsigned pr[kTunerPhases];
                    const unsigned nb = n0 + static_cast<unsigned>(cidx) * static_cast<unsigned>(kTunerPhases * D);
                    const bool whole = mb + kTunerPhases <= n_out;
                    if (sh >= 17 && sh <= 47) {
                        unsigned cl[kTunerPhases], pw[kTunerPhases];
#pragma unroll
                        for (int p = 0; p < kTunerPhases; p++) {
                            const int ar = acc[tt][p][0] + 256 * acc[tt][p][1], ai = acc[tt][p][2] + 256 * acc[tt][p][3];
                            const unsigned ph = w * (nb + static_cast<unsigned>(rb.nq[p]));
                            cl[p] = 0;
                            pw[p] = 0;
                            pr[p] = tuner_round_pair_fast(ar, ai, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh - 16, cl[p], pw[p]);
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
                            const unsigned ph = w * (nb + static_cast<unsigned>(rb.nq[p]));
                            unsigned cl = 0;
                            unsigned long long pw = 0;
                            pr[p] = tuner_round_pair(ar, ai, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh, cl, pw);
                            if (mb + p < n_out) {
                                clipped += cl;
                                power += pw;
                            }
                        }
                    }
                    rat_emit(obuf, via_lds, tt, g, col, u, U, out + static_cast<long>(ch) * pitch + 2 * mb, pr, whole, n_out - mb);
                }
            }
        }
        if (via_lds) {
            rat_wave_sync();
            rat_flush(obuf, out, pitch, grp, n_channels, c0, n_out, U, TT, lane);
            rat_wave_sync();
        }
    }
    tuner_add_levels(clipped, power, ch_ok && col == 0, levels + 2 * ch);
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
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = static_cast<int>(blockIdx.y) * 4 + wave;
    const int n_groups = (n_channels + kTunerGroup - 1) / kTunerGroup;
    const bool live = grp < n_groups;                               // wave-uniform
    const int col = lane & 15, g = lane >> 4;
    const int ch = grp * kTunerGroup + g;
    const bool ch_ok = live && ch < n_channels;
    const int n_pieces = 16 * TT * D + 4 * ks;                      // 16-byte pieces of a step's window, per plane
    uint8_t *stage_l = lds_raw + kTunerTableSize * 4;
    uint8_t *stage_h = stage_l + 16 * (n_pieces + n_pieces / D + 1);
    uint8_t *obuf = stage_h + 16 * (n_pieces + n_pieces / D + 1) + wave * (TT * 4 * 256 * U);   // this wave's output buffer (via_lds)

    for (int i = tid; i < kTunerTableSize; i += 256) tab[i] = table[i];

    unsigned w = 0;
    int sh = 1;
    if (ch_ok) {
        const uint2 cp = chan[ch];
        w = cp.x;
        sh = static_cast<int>(cp.y);
    }
    const int2 *kc_ch = kconst + static_cast<size_t>(ch_ok ? ch : 0) * U;
    const i4 *a_grp = a_img + static_cast<size_t>(live ? grp : 0) * kTunerPhases * U * ksp * 64 + lane;
    unsigned clipped = 0;
    unsigned long long power = 0;

    const int step0 = static_cast<int>(blockIdx.x) * steps_per_wg;
    for (int st = step0; st < step0 + steps_per_wg && st < n_steps; st++) {
        const long c0 = static_cast<long>(st) * (16 * TT);
        const long q0 = 16L * D * c0 - front;                       // plane position of the window's start, relative to the call
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
            const int off = 16 * (i + i / D);
            *reinterpret_cast<u4 *>(stage_l + off) = lo ^ 0x80808080u;   // low byte - 128 as int8
            *reinterpret_cast<u4 *>(stage_h + off) = hi;
        }
        __syncthreads();
        if (!live) continue;

        for (int u = 0; u < U; u++) {
            const RatBlock rb = rat_block(u, U, D, Tp, front);
            i4 accl[TT][kTunerPhases], acch[TT][kTunerPhases];
#pragma unroll
            for (int tt = 0; tt < TT; tt++)
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) accl[tt][p] = acch[tt][p] = i4{0, 0, 0, 0};
            const int jlo = rb.j0[0], jhi = rb.j1[kTunerPhases - 1];
            int rem = (4 * jlo + g) % D, blk = (4 * jlo + g) / D;   // (4 j + g) mod D and div D
            for (int j = jlo; j < jhi; j++) {
                i4 bl[TT], bh[TT];
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const int off = 16 * ((D + 1) * (16 * tt + col) + 4 * j + g + blk);
                    bl[tt] = *reinterpret_cast<const i4 *>(stage_l + off);
                    bh[tt] = *reinterpret_cast<const i4 *>(stage_h + off);
                }
                i4 a[kTunerPhases];
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    int jr = j - rb.j0[p];
                    jr = jr < 0 ? 0 : (jr >= ksp ? ksp - 1 : jr);
                    a[p] = a_grp[((kTunerPhases * u + p) * ksp + jr) * 64];
                }
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) {
                    if (j >= rb.j0[p] && j < rb.j1[p]) {
#pragma unroll
                        for (int tt = 0; tt < TT; tt++) {
                            accl[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], bl[tt], accl[tt][p], 0, 0, 0);
                            acch[tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], bh[tt], acch[tt][p], 0, 0, 0);
                        }
                    }
                }
                rem += 4;
                while (rem >= D) {
                    rem -= D;
                    blk++;
                }
            }
            if (ch_ok) {
                int2 kc[kTunerPhases];                              // the constants of the 8 images' phases
#pragma unroll
                for (int p = 0; p < kTunerPhases; p++) kc[p] = kc_ch[(kTunerPhases * u + p) * D % U];
#pragma unroll
                for (int tt = 0; tt < TT; tt++) {
                    const long cidx = c0 + 16 * tt + col;
                    const long mb = (cidx * U + u) * kTunerPhases;
                    if (mb >= n_out) continue;
                    unsigned pr[kTunerPhases];
                    const unsigned nb = n0 + static_cast<unsigned>(cidx) * static_cast<unsigned>(kTunerPhases * D);
                    const bool whole = mb + kTunerPhases <= n_out;
#pragma unroll
                    for (int p = 0; p < kTunerPhases; p++) {
                        const int lr = accl[tt][p][0] + 256 * accl[tt][p][1], li = accl[tt][p][2] + 256 * accl[tt][p][3];
                        const int hr = acch[tt][p][0] + 256 * acch[tt][p][1], hi = acch[tt][p][2] + 256 * acch[tt][p][3];
                        const unsigned ph = w * (nb + static_cast<unsigned>(rb.nq[p]));
                        unsigned cl = 0;
                        unsigned long long pw = 0;
                        pr[p] = tuner_round_pair_planes(lr, li, hr, hi, kc[p].x, kc[p].y, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh, cl, pw);
                        if (whole || mb + p < n_out) {
                            clipped += cl;
                            power += pw;
                        }
                    }
                    rat_emit(obuf, via_lds, tt, g, col, u, U, out + static_cast<long>(ch) * pitch + 2 * mb, pr, whole, n_out - mb);
                }
            }
        }
        if (via_lds) {
            rat_wave_sync();
            rat_flush(obuf, out, pitch, grp, n_channels, c0, n_out, U, TT, lane);
            rat_wave_sync();
        }
    }
    tuner_add_levels(clipped, power, ch_ok && col == 0, levels + 2 * ch);
}

constexpr size_t kTwoPerCu = 64 * 1024;     // the LDS a kernel may ask for without the attribute

template <typename K>
int rat_lds_attr(K kernel, size_t lds)
{
    if (lds > kTwoPerCu)
        FMRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    return FMRX_OK;
}

}  // namespace

int tuner_rat_mfma_launch(const TunerLaunch &a, long n_out, int n_steps, int steps_per_wg, dim3 grid, size_t lds, hipStream_t stream)
{
    const i4 *img = reinterpret_cast<const i4 *>(a.a_img);
#define FMRX_RAT_8(KERNEL)                                                                                                             \
    do {                                                                                                                               \
        FMRX_TRY(rat_lds_attr(KERNEL, lds));                                                                                           \
        hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, stream, a.x, a.hist, a.n_bytes, img, a.chan, a.table, a.out, a.pitch,         \
                           a.n_channels, n_out, a.U, a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, steps_per_wg, a.via_lds, a.levels); \
    } while (0)
#define FMRX_RAT_16(KERNEL)                                                                                                            \
    do {                                                                                                                               \
        FMRX_TRY(rat_lds_attr(KERNEL, lds));                                                                                           \
        hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, stream, a.x, a.hist, a.n_bytes, img, a.chan, a.kconst, a.table, a.out,        \
                           a.pitch, a.n_channels, n_out, a.U, a.D, a.Tp, a.front, a.ks, a.ksp, a.n0, n_steps, steps_per_wg, a.via_lds, \
                           a.levels);                                                                                                  \
    } while (0)
    if (a.format == kTunerS16) {
        if (a.tiles == 2)
            FMRX_RAT_16(tuner_rat_mfma_s16_kernel<2>);
        else
            FMRX_RAT_16(tuner_rat_mfma_s16_kernel<1>);
    } else if (a.format == kTunerS8) {
        if (a.tiles == 4)
            FMRX_RAT_8(tuner_rat_mfma_s8_kernel<4>);
        else if (a.tiles == 2)
            FMRX_RAT_8(tuner_rat_mfma_s8_kernel<2>);
        else
            FMRX_RAT_8(tuner_rat_mfma_s8_kernel<1>);
    } else {
        if (a.tiles == 4)
            FMRX_RAT_8(tuner_rat_mfma_kernel<4>);
        else if (a.tiles == 2)
            FMRX_RAT_8(tuner_rat_mfma_kernel<2>);
        else
            FMRX_RAT_8(tuner_rat_mfma_kernel<1>);
    }
#undef FMRX_RAT_8
#undef FMRX_RAT_16
    return FMRX_OK;
}

}  // namespace fmrx
