// blend.hip -- the stereo blend / soft mute stage's handle and C ABI (include/fmrx.h: fmrx_blend_*): per channel of a receiver
// bank, a stereo lamp, a blend towards mono and a mute, decided from the meters' pilot and noise powers and applied to the
// bank's audio.  Control step: blend_control.hpp; kernels: kernels_blend.hip; definition: tests/_blend_model.py (DESIGN.md
// section 4.12).
//
// The handle is meter_stage.hpp's stage behind the signal meters with the control structure: the stage owns no buffer of its own.
#include "blend_control.hpp"
#include "meter_stage.hpp"

using namespace fmrx;

struct fmrx_blend : meter_stage::MpxStage<fmrx_blend_status> {
    blend::Control control{};
};

namespace {

int launch(fmrx_blend *b, const meter_stage::Call<meter_stage::Mpx> &c)
{
    FMRX_TRY(blend_control_launch(b->control, c.src.d_mpx, c.src.d_seg_each, c.src.seg_all, b->d_status.p, b->n_channels, c.s));
    return blend_apply_launch(c.d_in, c.d_out, c.d_pcm, b->d_status.p, b->n_channels, b->audio_channels, b->n_audio, b->inv_n, c.wrap, c.s);
}

}  // namespace

extern "C" {

int fmrx_blend_defaults(fmrx_blend_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "blend_defaults: null argument");
    *p = fmrx_blend_params{20.0, 14.0, 20.0, 32.0, 10.0, 24.0, 0.0, 1.0, 0.25};
    return FMRX_OK;
}

int fmrx_blend_control(const fmrx_blend_params *p, double if_Fs, const fmrx_meter *rec, fmrx_blend_status *state_in_out)
{
    if (!p || !rec || !state_in_out) return fail(FMRX_EINVAL, "blend_control: null argument");
    blend::Control c;
    if (!blend::control_make(*p, if_Fs, &c)) return fail(FMRX_EINVAL, "blend_control: parameters (fmrx.h lists the conditions) or if_Fs %g", if_Fs);
    blend::control_step(c, rec->probe, rec->segments, *state_in_out);
    return FMRX_OK;
}

int fmrx_blend_create(fmrx_blend **out, const fmrx_blend_params *p, double if_Fs, int n_channels, int audio_channels, size_t n_audio, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "blend_create: null argument");
    blend::Control c;
    if (!blend::control_make(*p, if_Fs, &c)) return fail(FMRX_EINVAL, "blend_create: parameters (fmrx.h lists the conditions) or if_Fs %g", if_Fs);
    return meter_stage::create("blend_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_blend *b) -> int {
        b->control = c;
        return FMRX_OK;
    });
}

int fmrx_blend_destroy(fmrx_blend *b) { return meter_stage::destroy(b); }

int fmrx_blend_reset(fmrx_blend *b, int channel)
{
    return meter_stage::reset("blend_reset", b, channel, []() -> int { return FMRX_OK; });
}

int fmrx_blend_process_dev(fmrx_blend *b, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy, void *stream)
{
    return meter_stage::process_dev("blend_process_dev", b, launch, m, d_in, d_out, d_pcm16, pcm_policy, stream);
}

int fmrx_blend_process(fmrx_blend *b, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    return meter_stage::process("blend_process", b, launch, recs, in, out, pcm16, pcm_policy);
}

int fmrx_blend_status_get(fmrx_blend *b, fmrx_blend_status *out) { return meter_stage::status_get("blend_status_get", b, out); }

}  // extern "C"
