// tuner_mfma.hpp -- the pieces the wideband tuner's eleven matrix kernels are made of (kernels_tuner.hip: tuner_mfma_kernel,
// _s8_, _s16_; kernels_tuner_rational.hip: tuner_rat_mfma_kernel<4, 2, 1>, _s8_<4, 2, 1>, _s16_<2, 1>), in the order a kernel
// calls them:
//   tuner_wave, tuner_wave_setup   who this lane is; the rotation table into LDS, the channel's frequency word and shift
//   tuner_stage_bytes / _planes    a step's window into LDS: one plane of int8, or the 16-bit format's two byte planes
//   tuner_mac                      the K-step loop: 8 images x TT tiles x PLANES planes of v_mfma_i32_16x16x64_i8
//   tuner_finish8 / tuner_finish16 accumulators -> rotated, rounded (I, Q) pairs, clamps and power: the 8 outputs of a tile
//                                  (8-bit formats), one output (16-bit format)
//   tuner_launch_mfma              (host) the LDS attribute and the launch
// The layout they share is described at the head of kernels_tuner.hip.  What a kernel keeps is the order of the calls, where a
// K-step range and a phase word come from (once per kernel at an integer rate; rat_block(u) per block at a rational one) and
// where a piece goes (tuner_store_piece, or rat_emit / rat_flush).  D is the decimation in all of them (the integer tuner's R).
// Every device function is __forceinline__ in an anonymous namespace, like tuner_kernels.hpp's, whose rounding they end in.
// The compiler optimises such a function on its own before it inlines it, so what a piece updates many times it keeps in
// locals or takes and returns by value; three notes below say where that decided the form (profiles/tuner_kernels).
#pragma once
#include "tuner_kernels.hpp"

namespace fmrx {
namespace {

// A workgroup is 4 waves = 4 channel groups on one staged window; lane (col, g) of a wave holds column col of a tile and, in
// the C layout, channel g of the group.  live: the group exists (wave-uniform); ch_ok: the channel does.
struct TunerWave {
    int tid, lane, wave, grp, col, g, ch;
    bool live, ch_ok;
};
__device__ __forceinline__ TunerWave tuner_wave(int n_channels)
{
    TunerWave t;
    t.tid = threadIdx.x;
    t.lane = t.tid & 63;
    t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
    t.grp = static_cast<int>(blockIdx.y) * 4 + t.wave;
    t.live = t.grp < (n_channels + kTunerGroup - 1) / kTunerGroup;
    t.col = t.lane & 15;
    t.g = t.lane >> 4;
    t.ch = t.grp * kTunerGroup + t.g;
    t.ch_ok = t.live && t.ch < n_channels;
    return t;
}

// The rotation table into LDS (readable after the step loop's first __syncthreads), the channel's words {w, sh} (a lane without
// a channel rounds zeros with sh = 1), and the group's operand image: [image q < 8 U][ksp][64 lanes] from this lane's fragment.
__device__ __forceinline__ const i4 *tuner_wave_setup(const TunerWave &t, unsigned *tab, const unsigned *__restrict__ table,
                                                      const uint2 *__restrict__ chan, const i4 *__restrict__ a_img, int U, int ksp,
                                                      unsigned &w, int &sh)
{
    for (int i = t.tid; i < kTunerTableSize; i += 256) tab[i] = table[i];
    w = 0;
    sh = 1;
    if (t.ch_ok) {
        const uint2 cp = chan[t.ch];
        w = cp.x;
        sh = static_cast<int>(cp.y);
    }
    return a_img + static_cast<size_t>(t.live ? t.grp : 0) * kTunerPhases * U * ksp * 64 + t.lane;
}

// bytes of one staged plane of n_pieces 16-byte pieces, padded by one piece per D (tuner_lds_bytes counts the same)
__device__ __forceinline__ int tuner_plane_bytes(int n_pieces, int D) { return 16 * (n_pieces + n_pieces / D + 1); }

// A step's window of the 8-bit formats: n_pieces 16-byte pieces from byte q0 of the call (q < 0: the history's last `front`
// bytes; past n_bytes: zero samples), as int8, piece i at 16 (i + i / D): padded so that the 16 columns of a B read spread over
// the banks.  kFlip: what turns a raw byte into the int8 x (0x80 for unsigned bytes, 0 for signed ones) = the raw byte of a
// zero sample.
template <unsigned kFlip>
__device__ __forceinline__ void tuner_stage_bytes(uint8_t *stage, const uint8_t *__restrict__ x, const uint8_t *__restrict__ hist, long n_bytes,
                                                  int front, long q0, int n_pieces, int D, int tid)
{
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
}

// The 16-bit format's window as two byte planes.  x, hist: raw little-endian int16 I,Q values (n_values in the call, `front`
// in the history); a plane's byte u is value u's low or high byte, so plane positions (q0) are the 8-bit formats' byte
// positions and the raw position is twice that.  Low plane: low byte - 128 as int8; high plane: the int8 as it is.
__device__ __forceinline__ void tuner_stage_planes(uint8_t *stage_l, uint8_t *stage_h, const uint8_t *__restrict__ x,
                                                   const uint8_t *__restrict__ hist, long n_values, int front, long q0, int n_pieces, int D, int tid)
{
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
}

// The K-steps jlo .. jhi-1 of 8 images against TT tiles of PLANES staged planes: acc[plane][tile][image] = the products of the
// K-steps j0[p] <= j < j1[p] of image p.  This lane's B fragment of K-step j, tile tt is piece D (16 tt + col) + 4 j + g, padded
// by one piece per D; its A fragment of image p is a_first[(p ksp + j - j0[p]) 64] (an image outside its range loads its nearest
// stored step; the 8 loads are issued together), and every A fragment meets all the tiles and planes.  j0, j1, jlo, jhi are
// wave-uniform.
template <int TT, int PLANES>
__device__ __forceinline__ void tuner_mac(i4 (&acc_out)[PLANES][TT][kTunerPhases], const uint8_t *const (&stage)[PLANES],
                                          const i4 *__restrict__ a_first, const int (&j0)[kTunerPhases], const int (&j1)[kTunerPhases], int jlo,
                                          int jhi, int ksp, int D, int col, int g)
{
    // summed in locals and handed over at the end: the compiler optimises this function on its own before it inlines it, and
    // accumulators updated behind the reference come out of that as two copies of the registers (scratch at 4 tiles)
    i4 acc[PLANES][TT][kTunerPhases];
#pragma unroll
    for (int pl = 0; pl < PLANES; pl++)
#pragma unroll
        for (int tt = 0; tt < TT; tt++)
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) acc[pl][tt][p] = i4{0, 0, 0, 0};
    int rem = (4 * jlo + g) % D, blk = (4 * jlo + g) / D;       // (4 j + g) mod D and div D
    for (int j = jlo; j < jhi; j++) {
        i4 b[TT][PLANES];
#pragma unroll
        for (int tt = 0; tt < TT; tt++) {
            const int off = 16 * ((D + 1) * (16 * tt + col) + 4 * j + g + blk);
#pragma unroll
            for (int pl = 0; pl < PLANES; pl++) b[tt][pl] = *reinterpret_cast<const i4 *>(stage[pl] + off);
        }
        i4 a[kTunerPhases];
#pragma unroll
        for (int p = 0; p < kTunerPhases; p++) {
            int jr = j - j0[p];
            jr = jr < 0 ? 0 : (jr >= ksp ? ksp - 1 : jr);
            a[p] = a_first[(p * ksp + jr) * 64];
        }
#pragma unroll
        for (int p = 0; p < kTunerPhases; p++) {
            if (j >= j0[p] && j < j1[p]) {
#pragma unroll
                for (int tt = 0; tt < TT; tt++)
#pragma unroll
                    for (int pl = 0; pl < PLANES; pl++)
                        acc[pl][tt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b[tt][pl], acc[pl][tt][p], 0, 0, 0);
            }
        }
        rem += 4;
        while (rem >= D) {
            rem -= D;
            blk++;
        }
    }
#pragma unroll
    for (int pl = 0; pl < PLANES; pl++)
#pragma unroll
        for (int tt = 0; tt < TT; tt++)
#pragma unroll
            for (int p = 0; p < kTunerPhases; p++) acc_out[pl][tt][p] = acc[pl][tt][p];
}

// A tile's accumulators of the 8-bit formats -> the lane's 8 pairs pr[]: digits recombined, rotated by the table entry of
// phase word ph[p], rounded with shift sh in 32-bit arithmetic where 17 <= sh <= 47 and in 64-bit otherwise.  Clamps and power
// are counted for the outputs mb + p < n_out, those inside the call, only (whole: all 8 are).
__device__ __forceinline__ void tuner_finish8(const i4 (&acc)[kTunerPhases], const unsigned (&ph)[kTunerPhases], const unsigned *tab, int sh,
                                              bool whole, long mb, long n_out, unsigned (&pr)[kTunerPhases], unsigned &clipped, unsigned long long &power)
{
    if (sh >= 17 && sh <= 47) {
        unsigned cl[kTunerPhases], pw[kTunerPhases];
#pragma unroll
        for (int p = 0; p < kTunerPhases; p++) {
            const int ar = acc[p][0] + 256 * acc[p][1], ai = acc[p][2] + 256 * acc[p][3];
            cl[p] = 0;
            pw[p] = 0;
            pr[p] = tuner_round_pair_fast(ar, ai, rot_of(tab[ph[p] >> (32 - kTunerTableBits)]), sh - 16, cl[p], pw[p]);
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
        unsigned cs = 0;                                        // summed in locals: added behind the references, every `if` below
        unsigned long long ps = 0;                              // is a branch
#pragma unroll
        for (int p = 0; p < kTunerPhases; p++) {
            const int ar = acc[p][0] + 256 * acc[p][1], ai = acc[p][2] + 256 * acc[p][3];
            unsigned cl = 0;
            unsigned long long pw = 0;
            pr[p] = tuner_round_pair(ar, ai, rot_of(tab[ph[p] >> (32 - kTunerTableBits)]), sh, cl, pw);
            if (mb + p < n_out) {
                cs += cl;
                ps += pw;
            }
        }
        clipped += cs;
        power += ps;
    }
}

// One output of the 16-bit format: the two planes' accumulators and kc = the constant of the image's phase
// (tuner_round_pair_planes); counted: the output lies inside the call.  By value and per output: with the tile's arrays behind
// references, as tuner_finish8 has them, tuner_rat_mfma_s16_kernel<1> was 1 - 2 % slower.
__device__ __forceinline__ unsigned tuner_finish16(i4 accl, i4 acch, int2 kc, unsigned ph, const unsigned *tab, int sh, bool counted,
                                                   unsigned &clipped, unsigned long long &power)
{
    const int lr = accl[0] + 256 * accl[1], li = accl[2] + 256 * accl[3];
    const int hr = acch[0] + 256 * acch[1], hi = acch[2] + 256 * acch[3];
    unsigned cl = 0;
    unsigned long long pw = 0;
    const unsigned pr = tuner_round_pair_planes(lr, li, hr, hi, kc.x, kc.y, rot_of(tab[ph >> (32 - kTunerTableBits)]), sh, cl, pw);
    clipped += counted ? cl : 0u;                               // a select: behind the references an `if` becomes a branch per output
    power += counted ? pw : 0ull;
    return pr;
}

// Launch of a matrix kernel: 256 threads, `lds` bytes of dynamic LDS, asked for where it is more than a kernel gets without asking
template <typename K, typename... Args>
int tuner_launch_mfma(K kernel, dim3 grid, size_t lds, hipStream_t stream, Args... args)
{
    if (lds > kTwoPerCu)
        FMRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, args...);
    return FMRX_OK;
}

}  // namespace
}  // namespace fmrx
