// audio_resample_core.hpp -- the arithmetic of the audio rate converter (include/fmrx.h: fmrx_audio_resample_*; DESIGN.md section
// 4.19; defined by tests/_audio_resample_model.py): the limits of a geometry, the float32 tap table, the positions of a call's
// outputs, the mono mix and the fma chain of an output.  The host function fmrx_audio_resample_walk (audio_resample.hip) and the
// kernel (kernels_audio_resample.hip) compile these bodies, so the two cannot drift apart.
//
// An output is one chain: acc = +0, then acc = fmaf(h[p][j], x[i - j], acc) for j = 0 .. T - 1 ascending, one rounding per step.
// The chains of different outputs do not depend on each other, so two of them ride in the halves of one packed fma
// (v_pk_fma_f32 on the device) with every chain's own order and bits.  T is a multiple of 4 and a chain runs over exactly T taps:
// no chain is padded, so a non-finite sample reaches the outputs whose window holds it and no other.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fmrx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_AR_HD __host__ __device__ __forceinline__
#else
#define FMRX_AR_HD inline
#endif

namespace fmrx {
namespace audio_resample {

constexpr unsigned kMaxUp = 160, kMaxDown = 1024, kMinTaps = 8, kMaxTaps = 256, kMaxTable = 16384;
constexpr int kMaxCarry = 255;   // kMaxTaps - 1: the floats of a row in fmrx_audio_resample_state

using f2 = float __attribute__((ext_vector_type(2)));
using f4 = float __attribute__((ext_vector_type(4)));

inline unsigned gcd(unsigned a, unsigned b)
{
    while (b) {
        const unsigned t = a % b;
        a = b;
        b = t;
    }
    return a;
}

inline bool good_params(const fmrx_audio_resample_params *p)
{
    if (!p) return false;
    if (p->up < 1 || p->up > kMaxUp || p->down < 1 || p->down > kMaxDown || gcd(p->up, p->down) != 1) return false;
    if (p->taps < kMinTaps || p->taps > kMaxTaps || p->taps % 4 != 0 || p->up * p->taps > kMaxTable) return false;
    if (p->mix > 1) return false;
    if (!std::isfinite(p->cutoff) || !std::isfinite(p->beta)) return false;
    return p->cutoff > 0.0 && p->cutoff <= 1.0 && p->beta >= 0.0 && p->beta <= 20.0;
}

// the rows a channel converts
inline int rows_of(const fmrx_audio_resample_params &p, int audio_channels) { return p.mix ? 1 : audio_channels; }

// ceil(n up / down): the most outputs a call of n samples completes (pos = 0)
inline uint64_t max_out(uint64_t n, unsigned up, unsigned down) { return (n * up + down - 1) / down; }

// the outputs a call of n samples completes from position pos (0 .. down - 1)
FMRX_AR_HD uint64_t outputs_of(uint64_t n, unsigned up, unsigned down, unsigned pos)
{
    const uint64_t nu = n * up;
    return nu > pos ? (nu - pos + down - 1) / down : 0;
}

// I0 by its power series in double: sum ((x/2)^k / k!)^2; converges for every beta the limits allow
inline double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / (static_cast<double>(k) * static_cast<double>(k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// h[p][j] = g[j up + p], [up][taps] phase-major, made in double and rounded once
inline std::vector<float> make_taps(const fmrx_audio_resample_params &p)
{
    const unsigned U = p.up, T = p.taps, L = U * T;
    const double pi = 3.14159265358979323846;
    const double c = (static_cast<double>(L) - 1.0) / 2.0, half = static_cast<double>(L) / 2.0;
    const double ratio = static_cast<double>(U) / static_cast<double>(p.down);
    const double w = p.cutoff * (ratio < 1.0 ? ratio : 1.0), i0b = bessel_i0(p.beta);
    std::vector<float> h(L);
    for (unsigned k = 0; k < L; k++) {
        const double d = static_cast<double>(k) - c, a = pi * w * d / static_cast<double>(U), r = d / half;
        const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
        const double g = w * sinc * bessel_i0(p.beta * std::sqrt(1.0 - r * r)) / i0b;
        h[static_cast<size_t>(k % U) * T + k / U] = static_cast<float>(g);
    }
    return h;
}

// one float32 add and an exact halving, as the feature frames mix
FMRX_AR_HD float mono_mix(float l, float r) { return 0.5f * (l + r); }

// one output: h the T taps of its phase, newest the address of x[i]
FMRX_AR_HD float chain(const float *h, const float *newest, int T)
{
    float acc = 0.0f;
    for (int j = 0; j < T; j++) acc = fmaf(h[j], newest[-j], acc);
    return acc;
}

// four steps of two outputs' chains, in the halves of packed fmas: taps j .. j + 3 of each, and the samples x[i - j] .. x[i - j - 3]
FMRX_AR_HD f2 step4(f2 acc, const f4 ha, const f4 hb, const float (&xa)[4], const float (&xb)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) acc = __builtin_elementwise_fma(f2{ha[k], hb[k]}, f2{xa[k], xb[k]}, acc);
    return acc;
}

}  // namespace audio_resample
}  // namespace fmrx
