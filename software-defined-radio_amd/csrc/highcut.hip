// highcut.hip -- the variable high-cut stage's handle and C ABI (include/fmrx.h: fmrx_highcut_*): per channel of a receiver
// bank, a one-pole low-pass whose corner follows the channel's quieting, decided from the meters' noise powers and applied to
// the audio behind the blend (or behind the bank).  Control step: highcut_control.hpp; kernels: kernels_highcut.hip;
// definition: tests/_highcut_model.py.
//
// The handle keeps one status row per channel and one filter state per audio row on the device, the scratch of the parallel
// walk (the segments' start and end values, the miss counter), the event its last call recorded, a copy of the input for calls
// that run in place, an output for calls that take PCM only, and, for fmrx_highcut_process only, device copies of the host's
// records and rows.
#include "highcut_control.hpp"
#include "fmrx_internal.hpp"

using namespace fmrx;

struct fmrx_highcut {
    int device = 0, n_channels = 0, audio_channels = 0, L = kHighcutSegment, W = kHighcutWarmup;
    size_t n_audio = 0;
    float inv_n = 0.0f;
    bool force = false;
    highcut::Control control{};
    DevBuf<fmrx_highcut_status> d_status;
    DevBuf<float> d_state, d_seg;
    DevBuf<unsigned long long> d_missed;
    unsigned long long segments = 0;
    hipEvent_t done = nullptr;
    bool ran = false;
    DevBuf<float> d_copy, d_y;                // a call in place; a call with PCM only
    DevBuf<double> d_mpx;                     // fmrx_highcut_process only
    DevBuf<unsigned long long> d_segcount;
    DevBuf<float> d_in, d_out;
    DevBuf<int16_t> d_pcm;
    size_t rows() const { return static_cast<size_t>(n_channels) * audio_channels; }
    ~fmrx_highcut()
    {
        if (done) (void)hipEventDestroy(done);
    }
};

namespace {

constexpr size_t kSlack = 16;   // bytes in front of a device copy, so that it can take its host pointer's address modulo 16

int launch(fmrx_highcut *h, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all, const float *d_in,
           float *d_out, int16_t *d_pcm, int pcm_policy, hipStream_t s)
{
    const size_t total = h->rows() * h->n_audio;
    if (!d_out) {
        FMRX_TRY(h->d_y.ensure(total));      // (the first call that takes PCM only)
        d_out = h->d_y.p;
    }
    if (d_out == d_in) {                     // the walk reads its input again behind its own writes: it filters a copy
        FMRX_TRY(h->d_copy.ensure(total));   // (the first call in place)
        FMRX_HIP(hipMemcpyAsync(h->d_copy.p, d_in, total * sizeof(float), hipMemcpyDeviceToDevice, s));
        d_in = h->d_copy.p;
    }
    FMRX_TRY(highcut_control_launch(h->control, d_mpx, d_seg_each, seg_all, h->d_status.p, h->n_channels, s));
    HighcutArgs a;
    a.x = d_in;
    a.y = d_out;
    a.pcm = d_pcm;
    a.status = h->d_status.p;
    a.ac = h->audio_channels;
    a.wrap = pcm_policy == FMRX_PCM_WRAP ? 1 : 0;
    a.rows = h->rows();
    a.n = h->n_audio;
    a.inv_n = h->inv_n;
    a.p_max = h->control.p_max;
    a.L = h->L;
    a.W = h->W;
    a.state = h->d_state.p;
    a.seg = h->d_seg.p;
    a.missed = h->d_missed.p;
    FMRX_TRY(highcut_apply_launch(a, h->force, s, &h->segments));
    FMRX_HIP(hipEventRecord(h->done, s));
    h->ran = true;
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
    if (n_channels < 1) return fail(FMRX_EINVAL, "highcut_create: n_channels must be >= 1");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "highcut_create: audio_channels %d: 1 or 2", audio_channels);
    if (n_audio < 1 || n_audio > (size_t{1} << 26)) return fail(FMRX_EINVAL, "highcut_create: n_audio %zu: 1 .. 2^26", n_audio);
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    fmrx_highcut *h = new fmrx_highcut;
    h->device = device;
    h->n_channels = n_channels;
    h->audio_channels = audio_channels;
    h->n_audio = n_audio;
    h->inv_n = static_cast<float>(1.0 / static_cast<double>(n_audio));
    h->control = c;
    h->L = p->segment < 0 ? kHighcutSegment : p->segment;
    h->W = p->warmup < 0 ? kHighcutWarmup : p->warmup;
    auto body = [&]() -> int {
        FMRX_TRY(h->d_status.alloc(n_channels));
        FMRX_TRY(h->d_state.alloc(h->rows()));
        FMRX_TRY(h->d_seg.alloc(2 * h->rows() * static_cast<size_t>(highcut_segments(n_audio, h->L))));
        FMRX_TRY(h->d_missed.alloc(1));
        FMRX_HIP(hipMemset(h->d_status.p, 0, h->d_status.bytes()));
        FMRX_HIP(hipMemset(h->d_state.p, 0, h->d_state.bytes()));
        FMRX_HIP(hipMemset(h->d_missed.p, 0, h->d_missed.bytes()));
        FMRX_HIP(hipStreamSynchronize(nullptr));
        FMRX_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
        return FMRX_OK;
    };
    const int rc = body();
    if (rc != FMRX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return FMRX_OK;
}

int fmrx_highcut_destroy(fmrx_highcut *h)
{
    if (!h) return FMRX_OK;
    (void)hipSetDevice(h->device);
    if (h->ran) (void)hipEventSynchronize(h->done);
    delete h;
    return FMRX_OK;
}

int fmrx_highcut_reset(fmrx_highcut *h, int channel)
{
    if (!h) return fail(FMRX_EINVAL, "highcut_reset: null handle");
    if (channel >= h->n_channels) return fail(FMRX_EINVAL, "highcut_reset: channel %d of %d", channel, h->n_channels);
    FMRX_HIP(hipSetDevice(h->device));
    if (h->ran) FMRX_HIP(hipEventSynchronize(h->done));
    if (channel < 0) {
        FMRX_HIP(hipMemset(h->d_status.p, 0, h->d_status.bytes()));
        FMRX_HIP(hipMemset(h->d_state.p, 0, h->d_state.bytes()));
    } else {
        FMRX_HIP(hipMemset(h->d_status.p + channel, 0, sizeof(fmrx_highcut_status)));
        FMRX_HIP(hipMemset(h->d_state.p + static_cast<size_t>(channel) * h->audio_channels, 0, h->audio_channels * sizeof(float)));
    }
    FMRX_HIP(hipStreamSynchronize(nullptr));   // the rows are clear before this returns: a call on any stream, non-blocking ones included, finds them so
    return FMRX_OK;
}

int fmrx_highcut_set_force(fmrx_highcut *h, int on)
{
    if (!h) return fail(FMRX_EINVAL, "highcut_set_force: null handle");
    FMRX_HIP(hipSetDevice(h->device));
    if (h->ran) FMRX_HIP(hipEventSynchronize(h->done));
    h->force = on != 0;
    return FMRX_OK;
}

int fmrx_highcut_process_dev(fmrx_highcut *h, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy, void *stream)
{
    if (!h || !m) return fail(FMRX_EINVAL, "highcut_process_dev: null handle");
    FMRX_TRY(check_rows("highcut_process_dev", d_in, d_out, d_pcm16, pcm_policy));
    const MetersMpx v = meters_mpx(m);
    if (!v.ran || v.n_if == 0) return fail(FMRX_EINVAL, "highcut_process_dev: the meters' last call measured no discriminator rows");
    if (v.n_channels != h->n_channels || v.device != h->device)
        return fail(FMRX_EINVAL, "highcut_process_dev: the meters have %d channels on device %d, the high-cut %d on %d", v.n_channels, v.device,
                    h->n_channels, h->device);
    FMRX_HIP(hipSetDevice(h->device));
    return launch(h, v.d_mpx, nullptr, v.n_if / kMetersSegment, d_in, d_out, d_pcm16, pcm_policy, static_cast<hipStream_t>(stream));
}

int fmrx_highcut_process(fmrx_highcut *h, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    if (!h || !recs) return fail(FMRX_EINVAL, "highcut_process: null argument");
    FMRX_TRY(check_rows("highcut_process", in, out, pcm16, pcm_policy));
    FMRX_HIP(hipSetDevice(h->device));
    if (h->ran) FMRX_HIP(hipEventSynchronize(h->done));   // this call runs on the null stream: behind the handle's last call, whatever stream that was on
    const size_t N = h->n_channels, total = h->rows() * h->n_audio;
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
    FMRX_TRY(h->d_mpx.ensure(mpx.size()));
    FMRX_TRY(h->d_segcount.ensure(N));
    FMRX_HIP(hipMemcpy(h->d_mpx.p, mpx.data(), mpx.size() * sizeof(double), hipMemcpyHostToDevice));
    FMRX_HIP(hipMemcpy(h->d_segcount.p, seg.data(), N * sizeof(unsigned long long), hipMemcpyHostToDevice));
    // the device copies: at their host pointers' addresses modulo 16 (hipMalloc's are 256-byte aligned)
    const auto at = [](auto *base, const void *host) { return reinterpret_cast<decltype(base)>(reinterpret_cast<char *>(base) + (reinterpret_cast<uintptr_t>(host) & 15)); };
    FMRX_TRY(h->d_in.ensure(total + kSlack / sizeof(float)));
    float *d_in = at(h->d_in.p, in), *d_out = nullptr;
    int16_t *d_pcm = nullptr;
    FMRX_HIP(hipMemcpy(d_in, in, total * sizeof(float), hipMemcpyHostToDevice));
    if (out == in) d_out = d_in;
    else if (out) {
        FMRX_TRY(h->d_out.ensure(total + kSlack / sizeof(float)));
        d_out = at(h->d_out.p, out);
    }
    if (pcm16) {
        FMRX_TRY(h->d_pcm.ensure(total + kSlack / sizeof(int16_t)));
        d_pcm = at(h->d_pcm.p, pcm16);
    }
    FMRX_TRY(launch(h, h->d_mpx.p, h->d_segcount.p, 0, d_in, d_out, d_pcm, pcm_policy, nullptr));
    FMRX_HIP(hipEventSynchronize(h->done));
    if (out) FMRX_HIP(hipMemcpy(out, d_out, total * sizeof(float), hipMemcpyDeviceToHost));
    if (pcm16) FMRX_HIP(hipMemcpy(pcm16, d_pcm, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_highcut_status_get(fmrx_highcut *h, fmrx_highcut_status *out)
{
    if (!h || !out) return fail(FMRX_EINVAL, "highcut_status_get: null argument");
    FMRX_HIP(hipSetDevice(h->device));
    if (h->ran) FMRX_HIP(hipEventSynchronize(h->done));
    FMRX_HIP(hipMemcpy(out, h->d_status.p, static_cast<size_t>(h->n_channels) * sizeof(fmrx_highcut_status), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_highcut_diagnostics(fmrx_highcut *h, unsigned long long *segments, unsigned long long *missed)
{
    if (!h) return fail(FMRX_EINVAL, "highcut_diagnostics: null handle");
    FMRX_HIP(hipSetDevice(h->device));
    if (h->ran) FMRX_HIP(hipEventSynchronize(h->done));
    if (segments) *segments = h->segments;
    if (missed) FMRX_HIP(hipMemcpy(missed, h->d_missed.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

}  // extern "C"
