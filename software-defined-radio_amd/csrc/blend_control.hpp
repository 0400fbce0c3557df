// blend_control.hpp -- the control step of the stereo blend / soft mute stage (include/fmrx.h: fmrx_blend_*; DESIGN.md
// section 4.12): one channel's meter record and state -> lamp, targets, smoothed values and the float32 end points of the
// call's two ramps.  One definition for the host function (fmrx_blend_control, blend.hip) and the control kernel
// (blend_control_kernel, kernels_blend.hip); tests/_blend_model.py restates it in Python.
//
// Floating point: double add, subtract, multiply, divide, compare, frexp and the conversion to float only, one IEEE
// operation per step in a fixed order, FP contraction off -- host and device compute the same bits.  No sqrt and no log:
// neither is correctly rounded on both sides.  A compiler other than clang must be told itself not to contract (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "fmrx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_BHD __host__ __device__ __forceinline__
#else
#define FMRX_BHD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmrx {
namespace blend {

constexpr double kDbPerOctave = 3.010299956639812;   // the literal of the definition: dB = pseudo-log2 * this
constexpr double kSnap = 1.0 / 1024.0;               // a smoothed value this close to its target takes the target
constexpr double kRefHz = 7500.0;                    // the nominal pilot deviation the quieting ratio is referred to
constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
constexpr int kNoiseLo = 0, kNoiseHi = 1, kPilot = 2;   // the meters' probes (meters.hip: 17, 21 and 19 kHz)

// the parameters as the step uses them: thresholds in pseudo-log2, spans as reciprocals; made once on the host
struct Control {
    double pilot_on, pilot_off, blend_lo, blend_inv, mute_lo, mute_inv, floor, one_minus_floor, attack, release, ref1;
};

// false: the parameters are not valid (fmrx.h lists the conditions; NaN fails every one of them)
inline bool control_make(const fmrx_blend_params &p, double if_Fs, Control *c)
{
    const double v[9] = {p.pilot_on, p.pilot_off, p.blend_lo, p.blend_hi, p.mute_lo, p.mute_hi, p.mute_floor, p.attack, p.release};
    for (double x : v)
        if (!(x - x == 0.0)) return false;   // infinity or NaN
    if (!(if_Fs > 0.0) || !(if_Fs - if_Fs == 0.0)) return false;
    if (!(p.blend_hi > p.blend_lo) || !(p.mute_hi > p.mute_lo) || !(p.pilot_on >= p.pilot_off)) return false;
    if (!(p.mute_floor >= 0.0 && p.mute_floor <= 1.0)) return false;
    if (!(p.attack > 0.0 && p.attack <= 1.0) || !(p.release > 0.0 && p.release <= 1.0)) return false;
    c->pilot_on = p.pilot_on / kDbPerOctave;
    c->pilot_off = p.pilot_off / kDbPerOctave;
    c->blend_lo = p.blend_lo / kDbPerOctave;
    c->blend_inv = 1.0 / (p.blend_hi / kDbPerOctave - c->blend_lo);
    c->mute_lo = p.mute_lo / kDbPerOctave;
    c->mute_inv = 1.0 / (p.mute_hi / kDbPerOctave - c->mute_lo);
    c->floor = p.mute_floor;
    c->one_minus_floor = 1.0 - p.mute_floor;
    c->attack = p.attack;
    c->release = p.release;
    const double w = ((kTwoPi * kRefHz) / if_Fs) * 256.0;
    c->ref1 = w * w;
    return true;
}

// Mitchell's pseudo-logarithm: r = m 2^e, m in [1, 2) -> e + (m - 1).  frexp gives f = m / 2 and e + 1 exactly (subnormals
// included); 2 f - 1 is exact; the addition rounds once.  r finite and > 0.
FMRX_BHD double plog2(double r)
{
    int e;
    const double f = frexp(r, &e);
    return static_cast<double>(e - 1) + (2.0 * f - 1.0);
}

// the drive of a ratio, with the edge rule: -infinity reads lowest (ramp 0, lamp off), +infinity highest
FMRX_BHD double drive(double num, double den)
{
    const double inf = __builtin_inf();
    if (!(num > 0.0)) return -inf;
    if (!(den > 0.0)) return inf;
    const double r = num / den;
    if (!(r > 0.0)) return -inf;   // the quotient underflowed, or infinity / infinity
    if (r == inf) return inf;
    return plog2(r);
}

FMRX_BHD double ramp(double d, double lo, double inv_span)
{
    const double x = (d - lo) * inv_span;
    return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
}

FMRX_BHD double smooth(double s, double t, bool first, const Control &c)
{
    if (first) return t;
    const double k = t < s ? c.attack : c.release;
    const double v = s + k * (t - s);
    return fabs(t - v) <= kSnap ? t : v;
}

// probe: the record's probe[0 .. 5); st: the channel's state, replaced
FMRX_BHD void control_step(const Control &c, const double *probe, uint64_t segments, fmrx_blend_status &st)
{
    const double noise = (probe[kNoiseLo] + probe[kNoiseHi]) * 0.5;
    const double dp = drive(probe[kPilot], noise);
    const double dq = drive(c.ref1 * static_cast<double>(segments), noise);
    const bool first = st.calls == 0;
    const uint32_t kept = first ? 0u : st.lamp;
    const uint32_t lamp = dp >= c.pilot_on ? 1u : (dp < c.pilot_off ? 0u : kept);
    const double tb = lamp ? ramp(dp, c.blend_lo, c.blend_inv) : 0.0;
    const double tm = c.floor + c.one_minus_floor * ramp(dq, c.mute_lo, c.mute_inv);
    const double sb = smooth(st.sep, tb, first, c), sm = smooth(st.gain, tm, first, c);
    const float mono1 = static_cast<float>(1.0 - sb), gain1 = static_cast<float>(sm);
    st.mono0 = first ? mono1 : st.mono1;
    st.gain0 = first ? gain1 : st.gain1;
    st.mono1 = mono1;
    st.gain1 = gain1;
    st.pilot_db = dp * kDbPerOctave;
    st.quiet_db = dq * kDbPerOctave;
    st.sep_target = tb;
    st.gain_target = tm;
    st.sep = sb;
    st.gain = sm;
    st.lamp = lamp;
    st.reserved = 0;
    st.calls = st.calls + 1;
}

}  // namespace blend
}  // namespace fmrx
