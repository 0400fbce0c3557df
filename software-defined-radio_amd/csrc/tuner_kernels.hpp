// tuner_kernels.hpp -- the output side shared by the wideband tuner's kernels (kernels_tuner.hip, kernels_tuner_rational.hip),
// one sample or one lane at a time: the rotation-table entry, the rounding of a rotated sample to (I, Q) bytes in its three
// forms, the 16-byte store of a lane's 8 outputs and the level sums.  The generic kernel uses the first two; the matrix kernels
// reach all of it through the pieces of tuner_mfma.hpp.  Every function is __forceinline__ in an anonymous namespace.  Moving
// these helpers here left every kernel's code as it was (profiles/tuner_rational); the larger pieces of tuner_mfma.hpp do not
// promise that: profiles/tuner_kernels has what they did to each matrix kernel's code, registers and time.
#pragma once
#include "fmrx_internal.hpp"
#include "tuner_host.hpp"

namespace fmrx {
namespace {

using i4 = int __attribute__((ext_vector_type(4)));
using u4 = unsigned __attribute__((ext_vector_type(4)));

// one output sample: accumulator (ar, ai) -> rotated, rounded, clamped (I, Q) bytes; counts clamps and power
struct Rot {
    int c, s;
};
__device__ __forceinline__ Rot rot_of(unsigned t) { return {static_cast<short>(t & 0xffffu), static_cast<short>(t >> 16)}; }

// a rotated sample (yr, yi) -> rounded, clamped (I, Q) bytes
__device__ __forceinline__ unsigned tuner_round_y(long long yr, long long yi, int sh, unsigned &clipped, unsigned long long &power)
{
    const long long half = 1LL << (sh - 1);
    long long oi = 128 + ((yr + half) >> sh), oq = 128 + ((yi + half) >> sh);
    const long long ci = oi < 0 ? 0 : (oi > 255 ? 255 : oi), cq = oq < 0 ? 0 : (oq > 255 ? 255 : oq);
    clipped += (ci != oi) + (cq != oq);
    const int di = static_cast<int>(ci) - 128, dq = static_cast<int>(cq) - 128;
    power += static_cast<unsigned>(di * di + dq * dq);
    return static_cast<unsigned>(ci) | (static_cast<unsigned>(cq) << 8);
}

__device__ __forceinline__ unsigned tuner_round_pair(int ar, int ai, Rot r, int sh, unsigned &clipped, unsigned long long &power)
{
    const long long yr = static_cast<long long>(ar) * r.c + static_cast<long long>(ai) * r.s;
    const long long yi = static_cast<long long>(ai) * r.c - static_cast<long long>(ar) * r.s;
    return tuner_round_y(yr, yi, sh, clipped, power);
}

// The 16-bit format's pair: acc = k + l + 256 h per part (k the channel's constant, l and h the low and the high plane's
// sums, each an int32), |acc| < 2^40.  The rotation is taken term by term, every product int32 x int16 -> int64, so that
// nothing wider than a 32 x 32 -> 64 multiply-add is needed: |y| < 2^56.
__device__ __forceinline__ unsigned tuner_round_pair_planes(int lr, int li, int hr, int hi, int kr, int ki, Rot r, int sh, unsigned &clipped,
                                                            unsigned long long &power)
{
    const long long c = r.c, s = r.s;
    const long long yr = (lr * c + li * s) + (kr * c + ki * s) + 256 * (hr * c + hi * s);
    const long long yi = (li * c - lr * s) + (ki * c - kr * s) + 256 * (hi * c - hr * s);
    return tuner_round_y(yr, yi, sh, clipped, power);
}

// The same pair in 32-bit arithmetic, for 17 <= sh <= 47 (every gain a receiver would use): with a = ah 2^16 + al (al the
// balanced low half) the products by the 16-bit table entries are 24-bit multiplies, y = ph 2^16 + pl with |ph|, |pl| < 2^31,
// and since the rounding constant 2^(sh-1) is a multiple of 2^16,
//   (y + 2^(sh-1)) >> sh  =  (u + 2^(k-1)) >> k  =  (u >> k) + (bit k-1 of u),   u = ph + (pl >> 16) = y >> 16,  k = sh - 16:
// exactly the 64-bit form's result (nested floors of divisions by powers of two).
__device__ __forceinline__ int tuner_round_k(int ph, int pl, int k)
{
    const int u = ph + (pl >> 16);
    return 128 + (u >> k) + ((u >> (k - 1)) & 1);
}
__device__ __forceinline__ unsigned tuner_round_pair_fast(int ar, int ai, Rot r, int k, unsigned &clipped, unsigned &power)
{
    const int al = static_cast<short>(ar), bl = static_cast<short>(ai);
    const int ah = (ar - al) >> 16, bh = (ai - bl) >> 16;
    const int oi = tuner_round_k(__mul24(ah, r.c) + __mul24(bh, r.s), __mul24(al, r.c) + __mul24(bl, r.s), k);
    const int oq = tuner_round_k(__mul24(bh, r.c) - __mul24(ah, r.s), __mul24(bl, r.c) - __mul24(al, r.s), k);
    const int ci = min(max(oi, 0), 255), cq = min(max(oq, 0), 255);
    clipped += (ci != oi) + (cq != oq);
    const int di = ci - 128, dq = cq - 128;
    power += static_cast<unsigned>(di * di + dq * dq);
    return static_cast<unsigned>(ci) | (static_cast<unsigned>(cq) << 8);
}

// a lane's 8 consecutive (I, Q) pairs -> its 16-byte piece of the channel's row (n_left: outputs from this one to the call's end)
__device__ __forceinline__ void tuner_store_piece(uint8_t *dst, const unsigned (&pr)[kTunerPhases], bool whole, long n_left)
{
    if (whole) {
        *reinterpret_cast<u4 *>(dst) = u4{pr[0] | (pr[1] << 16), pr[2] | (pr[3] << 16), pr[4] | (pr[5] << 16), pr[6] | (pr[7] << 16)};
    } else {
#pragma unroll
        for (int p = 0; p < kTunerPhases; p++)
            if (p < n_left) *reinterpret_cast<unsigned short *>(dst + 2 * p) = static_cast<unsigned short>(pr[p]);
    }
}

// levels of the matrix kernels: the 16 columns of a channel sit in the 16 lanes of one quarter
__device__ __forceinline__ void tuner_add_levels(unsigned clipped, unsigned long long power, bool first_lane, unsigned long long *lv)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        clipped += __shfl_xor(clipped, o);
        power += __shfl_xor(power, o);
    }
    if (first_lane) {
        if (clipped) atomicAdd(lv, static_cast<unsigned long long>(clipped));
        if (power) atomicAdd(lv + 1, power);
    }
}

}  // namespace
}  // namespace fmrx
