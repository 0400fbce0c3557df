// leveller_control.hpp -- the control step of the loudness leveller / peak limiter stage (include/fmrx.h: fmrx_leveller_*;
// DESIGN.md section 4.15): one channel's audio meter record and state -> the loudness estimate, the gain and the float32 end
// points of the call's gain ramp; and the limiter's gain code of one sample.  One definition for the host functions
// (fmrx_leveller_control, fmrx_leveller_walk, leveller.hip) and the kernels (kernels_leveller.hip); tests/_leveller_model.py
// restates it in Python.
//
// Floating point: double add, subtract, multiply, divide, compare, frexp, ldexp, floor and the conversion to float only, one
// IEEE operation per step in a fixed order, FP contraction off -- host and device compute the same bits.  No sqrt, log or pow
// per call: the square root of the gain is Heron's iteration from a pseudo-logarithmic seed.  The parameters given in dB
// become linear values once, on the host, in control_make, with libm's pow -- the function the model's math.pow calls; the
// device only ever sees the results.  A compiler other than clang must be told itself not to contract (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "blend_control.hpp"   // FMRX_BHD, plog2

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmrx {
namespace leveller {

constexpr uint32_t kOne = FMRX_LEVELLER_ONE;          // the gain code of "no reduction", 2^24
constexpr int kMinLookahead = 8, kMaxLookahead = 128;
constexpr int kSpan = 2048;                            // samples a workgroup holds: its tile and 2 W in front
constexpr double kLkfsOffset = 0.691;                  // BS.1770: loudness = -0.691 + 10 log10(mean square)

// the parameters as the step uses them, made once on the host
struct Control {
    double fs2, target_ms, gate_ms, g_min, g_max, attack, release;
    float ceiling;
};

inline bool good_lookahead(int W) { return W >= kMinLookahead && W <= kMaxLookahead && (W & (W - 1)) == 0; }
inline int log2_of(int W)
{
    int s = 0;
    while ((1 << s) < W) s++;
    return s;
}

// false: the parameters are not valid (fmrx.h lists the conditions; NaN fails every one of them)
inline bool control_make(const fmrx_leveller_params &p, Control *c)
{
    const double v[8] = {p.target_lkfs, p.max_boost_db, p.max_cut_db, p.gate_lkfs, p.attack, p.release, p.ceiling_dbfs, p.full_scale};
    for (double x : v)
        if (!(x - x == 0.0)) return false;   // infinity or NaN
    if (!(p.max_boost_db >= 0.0) || !(p.max_cut_db >= 0.0) || !(p.gate_lkfs < p.target_lkfs)) return false;
    if (!(p.attack > 0.0 && p.attack <= 1.0) || !(p.release > 0.0 && p.release <= 1.0)) return false;
    if (!(p.ceiling_dbfs < 0.0) || !(p.full_scale > 0.0)) return false;
    volatile double ten = 10.0;   // pow itself, not what a compiler makes of pow(10.0, x)
    c->fs2 = p.full_scale * p.full_scale;
    c->target_ms = pow(ten, (p.target_lkfs + kLkfsOffset) / 10.0);
    c->gate_ms = pow(ten, (p.gate_lkfs + kLkfsOffset) / 10.0);
    c->g_max = pow(ten, p.max_boost_db / 20.0);
    c->g_min = pow(ten, -p.max_cut_db / 20.0);
    c->attack = p.attack;
    c->release = p.release;
    c->ceiling = static_cast<float>(p.full_scale * pow(ten, p.ceiling_dbfs / 20.0));
    const double w[5] = {c->fs2, c->target_ms, c->gate_ms, c->g_max, c->g_min};
    for (double x : w)
        if (!(x > 0.0) || !(x - x == 0.0)) return false;   // a level that left the doubles
    return c->ceiling >= 1.17549435e-38f && c->ceiling - c->ceiling == 0.0f;   // a normal float
}

// 2^x with the fraction read linearly, the inverse of plog2: (1 + (x - floor x)) 2^(floor x)
FMRX_BHD double pexp2(double x)
{
    const double f = floor(x);
    return ldexp(1.0 + (x - f), static_cast<int>(f));
}

// the square root of a finite r > 0: the seed is within 6 % (Mitchell's error, halved, and the linear 2^x's), two Heron steps
// square that twice: 1.5e-6 measured (tests/test_leveller_model_host.py)
FMRX_BHD double heron2(double r)
{
    double y = pexp2(0.5 * blend::plog2(r));
    y = 0.5 * (y + r / y);
    y = 0.5 * (y + r / y);
    return y;
}

// n, k2a, k2b: the record's n and sum_k2[0 .. 2); st: the channel's state, replaced
FMRX_BHD void control_step(const Control &c, int ac, uint64_t n, double k2a, double k2b, fmrx_leveller_status &st)
{
    const double inf = __builtin_inf();
    const double k2 = k2a + (ac == 2 ? k2b : 0.0);
    const double ms = (k2 / static_cast<double>(n)) / c.fs2;
    const bool gated = !(ms >= c.gate_ms && ms < inf);
    double loud = st.loud_ms;
    if (!gated) {
        if (!(loud > 0.0)) loud = ms;
        else {
            const double k = ms > loud ? c.attack : c.release;
            loud = loud + k * (ms - loud);
        }
    }
    double gain = 1.0;
    if (loud > 0.0) {
        const double r = c.target_ms / loud;
        if (!(r > 0.0)) gain = c.g_min;
        else if (r == inf) gain = c.g_max;
        else {
            const double y = heron2(r);
            gain = y < c.g_min ? c.g_min : (y > c.g_max ? c.g_max : y);
        }
    }
    const float gain1 = static_cast<float>(gain);
    st.gain0 = st.calls == 0 ? gain1 : st.gain1;
    st.gain1 = gain1;
    st.loud_ms = loud;
    st.gain = gain;
    st.gated = gated ? 1u : 0u;
    st.min_code = kOne;   // the apply pass lowers and counts
    st.limited = 0;
    st.reserved = 0;
    st.calls = st.calls + 1;
}

// the gain code of a magnitude a = |u| under the ceiling c: one float divide, one float multiply, truncation
FMRX_BHD uint32_t code_of(float a, float c)
{
    if (a <= c) return kOne;
    if (!(a < __builtin_inff())) return 0u;   // NaN and infinity
    return static_cast<uint32_t>((c / a) * 16777216.0f);
}

}  // namespace leveller
}  // namespace fmrx
