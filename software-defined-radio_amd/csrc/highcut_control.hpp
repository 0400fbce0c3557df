// highcut_control.hpp -- the design and the control step of the variable high-cut stage (include/fmrx.h: fmrx_highcut_*;
// DESIGN.md section 4.13): one channel's meter record and state -> openness target, smoothed openness and the float32 end
// points (p0, p1) of the call's pole ramp.  One definition for the host function (fmrx_highcut_control, highcut.hip) and the
// control kernel (highcut_control_kernel, kernels_highcut.hip); tests/_highcut_model.py restates it in Python.
//
// The arithmetic is the blend's (blend_control.hpp: drive, plog2, ramp, smooth and its constants, used as they are), under the
// same floating-point rules: one IEEE double operation per step in a fixed order, FP contraction off.  The only
// transcendental, exp in the design of p_max, runs once on the host.
#pragma once
#include "blend_control.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmrx {
namespace highcut {

constexpr float kPoleCap = 0.875f;   // the largest p_max: beyond it the built-in lanes' warm-up no longer meets the serial walk on ordinary audio

// the parameters as the step uses them; made once on the host.  b: attack, release and ref1 in the blend's own structure, for
// its smooth(); the blend's other fields are not read
struct Control {
    blend::Control b;
    double hc_lo, hc_inv, floor, cut_max, p_max_d;
    float p_max;
};

// false: fc_min or audio_Fs is not valid (not finite, not > 0, or a p_max above the cap)
inline bool design(double fc_min, double audio_Fs, double *p_max_d, float *p_max)
{
    if (!(fc_min - fc_min == 0.0) || !(audio_Fs - audio_Fs == 0.0) || !(fc_min > 0.0) || !(audio_Fs > 0.0)) return false;
    const double d = exp(((-blend::kTwoPi) * fc_min) / audio_Fs);
    const float f = static_cast<float>(d);
    if (!(f <= kPoleCap)) return false;
    *p_max_d = d;
    *p_max = f;
    return true;
}

// false: the parameters are not valid (fmrx.h lists the conditions; NaN fails every one of them)
inline bool control_make(const fmrx_highcut_params &p, double if_Fs, double audio_Fs, Control *c)
{
    const double v[6] = {p.fc_min, p.hc_lo, p.hc_hi, p.cut_max, p.attack, p.release};
    for (double x : v)
        if (!(x - x == 0.0)) return false;   // infinity or NaN
    if (!(if_Fs > 0.0) || !(if_Fs - if_Fs == 0.0)) return false;
    if (!(p.hc_hi > p.hc_lo) || !(p.cut_max >= 0.0 && p.cut_max <= 1.0)) return false;
    if (!(p.attack > 0.0 && p.attack <= 1.0) || !(p.release > 0.0 && p.release <= 1.0)) return false;
    if (p.warmup < -1 || p.warmup > (1 << 20) || p.segment < -1 || p.segment == 0 || p.segment > (1 << 20)) return false;
    *c = Control{};
    if (!design(p.fc_min, audio_Fs, &c->p_max_d, &c->p_max)) return false;
    c->hc_lo = p.hc_lo / blend::kDbPerOctave;
    c->hc_inv = 1.0 / (p.hc_hi / blend::kDbPerOctave - c->hc_lo);
    c->floor = 1.0 - p.cut_max;
    c->cut_max = p.cut_max;
    c->b.attack = p.attack;
    c->b.release = p.release;
    const double w = ((blend::kTwoPi * blend::kRefHz) / if_Fs) * 256.0;
    c->b.ref1 = w * w;
    return true;
}

// probe: the record's probe[0 .. 5); st: the channel's state, replaced
FMRX_BHD void control_step(const Control &c, const double *probe, uint64_t segments, fmrx_highcut_status &st)
{
    const double noise = (probe[blend::kNoiseLo] + probe[blend::kNoiseHi]) * 0.5;
    const double dq = blend::drive(c.b.ref1 * static_cast<double>(segments), noise);
    const bool first = st.calls == 0;
    const double t = c.floor + c.cut_max * blend::ramp(dq, c.hc_lo, c.hc_inv);
    const double s = blend::smooth(st.open, t, first, c.b);
    const float p1 = static_cast<float>((1.0 - s) * c.p_max_d);
    st.p0 = first ? p1 : st.p1;
    st.p1 = p1;
    st.quiet_db = dq * blend::kDbPerOctave;
    st.open_target = t;
    st.open = s;
    st.calls = st.calls + 1;
}

}  // namespace highcut
}  // namespace fmrx
