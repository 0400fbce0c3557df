// blend.hip -- the stereo blend / soft mute stage's handle and C ABI (include/fmrx.h: fmrx_blend_*): per channel of a receiver
// bank, a stereo lamp, a blend towards mono and a mute, decided from the meters' pilot and noise powers and applied to the
// bank's audio.  Control step: blend_control.hpp; kernels: kernels_blend.hip; definition: tests/_blend_model.py (DESIGN.md
// section 4.12).
//
// The handle keeps one status row per channel on the device -- state and result at once --, the event its last call recorded,
// and, for fmrx_blend_process only, device copies of the host's records and rows.
#include "blend_control.hpp"
#include "fmrx_internal.hpp"

using namespace fmrx;

struct fmrx_blend {
    int device = 0, n_channels = 0, audio_channels = 0;
    size_t n_audio = 0;
    float inv_n = 0.0f;
    blend::Control control{};
    DevBuf<fmrx_blend_status> d_status;
    hipEvent_t done = nullptr;
    bool ran = false;
    DevBuf<double> d_mpx;                     // fmrx_blend_process only
    DevBuf<unsigned long long> d_seg;
    DevBuf<float> d_in, d_out;
    DevBuf<int16_t> d_pcm;
    ~fmrx_blend()
    {
        if (done) (void)hipEventDestroy(done);
    }
};

namespace {

constexpr size_t kSlack = 16;   // bytes in front of a device copy, so that it can take its host pointer's address modulo 16

int launch(fmrx_blend *b, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all, const float *d_in,
           float *d_out, int16_t *d_pcm, int pcm_policy, hipStream_t s)
{
    FMRX_TRY(blend_control_launch(b->control, d_mpx, d_seg_each, seg_all, b->d_status.p, b->n_channels, s));
    FMRX_TRY(blend_apply_launch(d_in, d_out, d_pcm, b->d_status.p, b->n_channels, b->audio_channels, b->n_audio, b->inv_n,
                                pcm_policy == FMRX_PCM_WRAP ? 1 : 0, s));
    FMRX_HIP(hipEventRecord(b->done, s));
    b->ran = true;
    return FMRX_OK;
}

int check_rows(const char *who, const float *in, const float *out, const int16_t *pcm, int pcm_policy)
{
    if (!in) return fail(FMRX_EINVAL, "%s: null input", who);
    if (!out && !pcm) return fail(FMRX_EINVAL, "%s: neither float nor PCM output", who);
    if (reinterpret_cast<uintptr_t>(in) % sizeof(float) || reinterpret_cast<uintptr_t>(out) % sizeof(float) || reinterpret_cast<uintptr_t>(pcm) % sizeof(int16_t))
        return fail(FMRX_EINVAL, "%s: float rows must be 4-byte aligned, PCM 2-byte", who);
    if (pcm_policy != FMRX_PCM_WRAP && pcm_policy != FMRX_PCM_SATURATE) return fail(FMRX_EINVAL, "%s: pcm_policy %d", who, pcm_policy);
    return FMRX_OK;
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
    if (n_channels < 1) return fail(FMRX_EINVAL, "blend_create: n_channels must be >= 1");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "blend_create: audio_channels %d: 1 or 2", audio_channels);
    if (n_audio < 1 || n_audio > (size_t{1} << 26)) return fail(FMRX_EINVAL, "blend_create: n_audio %zu: 1 .. 2^26", n_audio);
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    fmrx_blend *b = new fmrx_blend;
    b->device = device;
    b->n_channels = n_channels;
    b->audio_channels = audio_channels;
    b->n_audio = n_audio;
    b->inv_n = static_cast<float>(1.0 / static_cast<double>(n_audio));
    b->control = c;
    auto body = [&]() -> int {
        FMRX_TRY(b->d_status.alloc(n_channels));
        FMRX_HIP(hipMemset(b->d_status.p, 0, b->d_status.bytes()));
        FMRX_HIP(hipStreamSynchronize(nullptr));
        FMRX_HIP(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
        return FMRX_OK;
    };
    const int rc = body();
    if (rc != FMRX_OK) {
        delete b;
        return rc;
    }
    *out = b;
    return FMRX_OK;
}

int fmrx_blend_destroy(fmrx_blend *b)
{
    if (!b) return FMRX_OK;
    (void)hipSetDevice(b->device);
    if (b->ran) (void)hipEventSynchronize(b->done);
    delete b;
    return FMRX_OK;
}

int fmrx_blend_reset(fmrx_blend *b, int channel)
{
    if (!b) return fail(FMRX_EINVAL, "blend_reset: null handle");
    if (channel >= b->n_channels) return fail(FMRX_EINVAL, "blend_reset: channel %d of %d", channel, b->n_channels);
    FMRX_HIP(hipSetDevice(b->device));
    if (b->ran) FMRX_HIP(hipEventSynchronize(b->done));
    if (channel < 0) FMRX_HIP(hipMemset(b->d_status.p, 0, b->d_status.bytes()));
    else FMRX_HIP(hipMemset(b->d_status.p + channel, 0, sizeof(fmrx_blend_status)));
    FMRX_HIP(hipStreamSynchronize(nullptr));   // the rows are clear before this returns: a call on any stream, non-blocking ones included, finds them so
    return FMRX_OK;
}

int fmrx_blend_process_dev(fmrx_blend *b, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy, void *stream)
{
    if (!b || !m) return fail(FMRX_EINVAL, "blend_process_dev: null handle");
    FMRX_TRY(check_rows("blend_process_dev", d_in, d_out, d_pcm16, pcm_policy));
    const MetersMpx v = meters_mpx(m);
    if (!v.ran || v.n_if == 0) return fail(FMRX_EINVAL, "blend_process_dev: the meters' last call measured no discriminator rows");
    if (v.n_channels != b->n_channels || v.device != b->device)
        return fail(FMRX_EINVAL, "blend_process_dev: the meters have %d channels on device %d, the blend %d on %d", v.n_channels, v.device,
                    b->n_channels, b->device);
    FMRX_HIP(hipSetDevice(b->device));
    return launch(b, v.d_mpx, nullptr, v.n_if / kMetersSegment, d_in, d_out, d_pcm16, pcm_policy, static_cast<hipStream_t>(stream));
}

int fmrx_blend_process(fmrx_blend *b, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    if (!b || !recs) return fail(FMRX_EINVAL, "blend_process: null argument");
    FMRX_TRY(check_rows("blend_process", in, out, pcm16, pcm_policy));
    FMRX_HIP(hipSetDevice(b->device));
    if (b->ran) FMRX_HIP(hipEventSynchronize(b->done));   // this call runs on the null stream: behind the handle's last call, whatever stream that was on
    const size_t N = b->n_channels, total = N * b->audio_channels * b->n_audio;
    std::vector<double> mpx(N * kMetersMpxFields, 0.0);
    std::vector<unsigned long long> seg(N);
    for (size_t c = 0; c < N; c++) {
        double *o = mpx.data() + c * kMetersMpxFields;
        o[0] = recs[c].sum_x;
        o[1] = recs[c].sum_x2;
        o[2] = recs[c].max_abs;
        for (int p = 0; p < kMetersProbes; p++) o[3 + p] = recs[c].probe[p];
        seg[c] = recs[c].segments;
    }
    FMRX_TRY(b->d_mpx.ensure(mpx.size()));
    FMRX_TRY(b->d_seg.ensure(N));
    FMRX_HIP(hipMemcpy(b->d_mpx.p, mpx.data(), mpx.size() * sizeof(double), hipMemcpyHostToDevice));
    FMRX_HIP(hipMemcpy(b->d_seg.p, seg.data(), N * sizeof(unsigned long long), hipMemcpyHostToDevice));
    // the device copies: at their host pointers' addresses modulo 16 (hipMalloc's are 256-byte aligned)
    const auto at = [](auto *base, const void *host) { return reinterpret_cast<decltype(base)>(reinterpret_cast<char *>(base) + (reinterpret_cast<uintptr_t>(host) & 15)); };
    FMRX_TRY(b->d_in.ensure(total + kSlack / sizeof(float)));
    float *d_in = at(b->d_in.p, in), *d_out = nullptr;
    int16_t *d_pcm = nullptr;
    FMRX_HIP(hipMemcpy(d_in, in, total * sizeof(float), hipMemcpyHostToDevice));
    if (out == in) d_out = d_in;
    else if (out) {
        FMRX_TRY(b->d_out.ensure(total + kSlack / sizeof(float)));
        d_out = at(b->d_out.p, out);
    }
    if (pcm16) {
        FMRX_TRY(b->d_pcm.ensure(total + kSlack / sizeof(int16_t)));
        d_pcm = at(b->d_pcm.p, pcm16);
    }
    FMRX_TRY(launch(b, b->d_mpx.p, b->d_seg.p, 0, d_in, d_out, d_pcm, pcm_policy, nullptr));
    FMRX_HIP(hipEventSynchronize(b->done));
    if (out) FMRX_HIP(hipMemcpy(out, d_out, total * sizeof(float), hipMemcpyDeviceToHost));
    if (pcm16) FMRX_HIP(hipMemcpy(pcm16, d_pcm, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_blend_status_get(fmrx_blend *b, fmrx_blend_status *out)
{
    if (!b || !out) return fail(FMRX_EINVAL, "blend_status_get: null argument");
    FMRX_HIP(hipSetDevice(b->device));
    if (b->ran) FMRX_HIP(hipEventSynchronize(b->done));
    FMRX_HIP(hipMemcpy(out, b->d_status.p, static_cast<size_t>(b->n_channels) * sizeof(fmrx_blend_status), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

}  // extern "C"
