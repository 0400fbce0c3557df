// highcut.hip -- the variable high-cut stage's handle and C ABI (include/fmrx.h: fmrx_highcut_*): per channel of a receiver
// bank, a one-pole low-pass whose corner follows the channel's quieting, decided from the meters' noise powers and applied to
// the audio behind the blend (or behind the bank).  Control step: highcut_control.hpp; kernels: kernels_highcut.hip;
// definition: tests/_highcut_model.py.
//
// The handle is meter_stage.hpp's stage behind the signal meters with the control structure, one filter state per audio row on
// the device, the scratch of the parallel walk (the segments' start and end values, the miss counter), a copy of the input for
// calls that run in place and an output for calls that take PCM only.
#include "highcut_control.hpp"
#include "meter_stage.hpp"

using namespace fmrx;

struct fmrx_highcut : meter_stage::MpxStage<fmrx_highcut_status> {
    int L = kHighcutSegment, W = kHighcutWarmup;
    bool force = false;
    highcut::Control control{};
    DevBuf<float> d_state, d_seg;
    DevBuf<unsigned long long> d_missed;
    unsigned long long segments = 0;
    DevBuf<float> d_copy, d_y;                // a call in place; a call with PCM only
};

namespace {

int launch(fmrx_highcut *h, const meter_stage::Call<meter_stage::Mpx> &c)
{
    const size_t total = h->rows() * h->n_audio;
    HighcutArgs a;
    a.x = c.d_in;
    a.y = c.d_out;
    if (!a.y) {
        FMRX_TRY(h->d_y.ensure(total));      // (the first call that takes PCM only)
        a.y = h->d_y.p;
    }
    if (a.y == a.x) {                        // the walk reads its input again behind its own writes: it filters a copy
        FMRX_TRY(h->d_copy.ensure(total));   // (the first call in place)
        FMRX_HIP(hipMemcpyAsync(h->d_copy.p, a.x, total * sizeof(float), hipMemcpyDeviceToDevice, c.s));
        a.x = h->d_copy.p;
    }
    FMRX_TRY(highcut_control_launch(h->control, c.src.d_mpx, c.src.d_seg_each, c.src.seg_all, h->d_status.p, h->n_channels, c.s));
    a.pcm = c.d_pcm;
    a.status = h->d_status.p;
    a.ac = h->audio_channels;
    a.wrap = c.wrap;
    a.rows = h->rows();
    a.n = h->n_audio;
    a.inv_n = h->inv_n;
    a.p_max = h->control.p_max;
    a.L = h->L;
    a.W = h->W;
    a.state = h->d_state.p;
    a.seg = h->d_seg.p;
    a.missed = h->d_missed.p;
    return highcut_apply_launch(a, h->force, c.s, &h->segments);
}

}  // namespace

extern "C" {

int fmrx_highcut_defaults(fmrx_highcut_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "highcut_defaults: null argument");
    *p = fmrx_highcut_params{2500.0, 16.0, 36.0, 1.0, 1.0, 0.25, -1, -1};
    return FMRX_OK;
}

int fmrx_highcut_design(double fc_min, double audio_Fs, float *p_max)
{
    if (!p_max) return fail(FMRX_EINVAL, "highcut_design: null argument");
    double d;
    if (!highcut::design(fc_min, audio_Fs, &d, p_max))
        return fail(FMRX_EINVAL, "highcut_design: fc_min %g and audio_Fs %g must be finite and > 0 and give a pole of at most 0.875", fc_min, audio_Fs);
    return FMRX_OK;
}

int fmrx_highcut_control(const fmrx_highcut_params *p, double if_Fs, double audio_Fs, const fmrx_meter *rec, fmrx_highcut_status *state_in_out)
{
    if (!p || !rec || !state_in_out) return fail(FMRX_EINVAL, "highcut_control: null argument");
    highcut::Control c;
    if (!highcut::control_make(*p, if_Fs, audio_Fs, &c))
        return fail(FMRX_EINVAL, "highcut_control: parameters (fmrx.h lists the conditions), if_Fs %g or audio_Fs %g", if_Fs, audio_Fs);
    highcut::control_step(c, rec->probe, rec->segments, *state_in_out);
    return FMRX_OK;
}

int fmrx_highcut_create(fmrx_highcut **out, const fmrx_highcut_params *p, double if_Fs, double audio_Fs, int n_channels, int audio_channels,
                        size_t n_audio, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "highcut_create: null argument");
    highcut::Control c;
    if (!highcut::control_make(*p, if_Fs, audio_Fs, &c))
        return fail(FMRX_EINVAL, "highcut_create: parameters (fmrx.h lists the conditions), if_Fs %g or audio_Fs %g", if_Fs, audio_Fs);
    return meter_stage::create("highcut_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_highcut *h) -> int {
        h->control = c;
        h->L = p->segment < 0 ? kHighcutSegment : p->segment;
        h->W = p->warmup < 0 ? kHighcutWarmup : p->warmup;
        FMRX_TRY(h->d_state.alloc(h->rows()));
        FMRX_TRY(h->d_seg.alloc(2 * h->rows() * static_cast<size_t>(highcut_segments(n_audio, h->L))));
        FMRX_TRY(h->d_missed.alloc(1));
        FMRX_HIP(hipMemset(h->d_state.p, 0, h->d_state.bytes()));
        FMRX_HIP(hipMemset(h->d_missed.p, 0, h->d_missed.bytes()));
        return FMRX_OK;
    });
}

int fmrx_highcut_destroy(fmrx_highcut *h) { return meter_stage::destroy(h); }

int fmrx_highcut_reset(fmrx_highcut *h, int channel)
{
    return meter_stage::reset("highcut_reset", h, channel, [&]() -> int {   // the filter state of the channel's rows with its status
        if (channel < 0) FMRX_HIP(hipMemset(h->d_state.p, 0, h->d_state.bytes()));
        else FMRX_HIP(hipMemset(h->d_state.p + static_cast<size_t>(channel) * h->audio_channels, 0, h->audio_channels * sizeof(float)));
        return FMRX_OK;
    });
}

int fmrx_highcut_set_force(fmrx_highcut *h, int on)
{
    if (!h) return fail(FMRX_EINVAL, "highcut_set_force: null handle");
    FMRX_TRY(h->wait());
    h->force = on != 0;
    return FMRX_OK;
}

int fmrx_highcut_process_dev(fmrx_highcut *h, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy, void *stream)
{
    return meter_stage::process_dev("highcut_process_dev", h, launch, m, d_in, d_out, d_pcm16, pcm_policy, stream);
}

int fmrx_highcut_process(fmrx_highcut *h, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    return meter_stage::process("highcut_process", h, launch, recs, in, out, pcm16, pcm_policy);
}

int fmrx_highcut_status_get(fmrx_highcut *h, fmrx_highcut_status *out) { return meter_stage::status_get("highcut_status_get", h, out); }

int fmrx_highcut_diagnostics(fmrx_highcut *h, unsigned long long *segments, unsigned long long *missed)
{
    if (!h) return fail(FMRX_EINVAL, "highcut_diagnostics: null handle");
    FMRX_TRY(h->wait());
    if (segments) *segments = h->segments;
    if (missed) FMRX_HIP(hipMemcpy(missed, h->d_missed.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

}  // extern "C"
