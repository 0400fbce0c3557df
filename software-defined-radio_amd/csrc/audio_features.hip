// audio_features.hip -- the audio feature frames' handle, host arithmetic and C ABI (include/fmrx.h: fmrx_audio_features_*): per
// channel of a receiver bank, a mel-band spectrogram of the channel's mono mix, one row of n_mels linear powers per frame of win
// samples every hop samples, left on the device as [n_channels][F_max][n_mels].  Kernel: kernels_audio_features.hip; the tables
// and the frame arithmetic, shared with fmrx_audio_features_walk below: audio_features_core.hpp; definition:
// tests/_audio_features_model.py.
//
// A reader of meter_stage.hpp: it only reads the rows.  Its own part is the geometry and its tables on the device, the carried
// state on the device in two pairs of buffers, one read and one written per call (channel-major: fill, and win floats of the mono
// mix per channel), the results a call writes (the features and the frames per channel, which stay on the device until a collect
// asks for them) and the host arithmetic.
#include "meter_stage.hpp"
#include "audio_features_core.hpp"

#include <cmath>

using namespace fmrx;

struct fmrx_audio_features : meter_stage::Reader {
    fmrx_audio_features_params p = {};
    size_t f_max = 0;
    DevBuf<float> d_w, d_c, d_mel_w;
    DevBuf<int> d_lo, d_hi;
    DevBuf<unsigned> d_fill[2];
    DevBuf<float> d_carry[2];    // [n_channels][win]
    int cur = 0;                 // the buffers the next call reads
    DevBuf<unsigned> d_frames;
    DevBuf<float> d_feat;        // [n_channels][f_max][n_mels]
};

namespace {

constexpr int kMaxWin = audio_features::kMaxWin;

int take_params(const char *who, const fmrx_audio_features_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (!audio_features::good_params(p))
        return fail(FMRX_EINVAL,
                    "%s: win %u (a multiple of 4, 16 .. 1280), hop %u (1 .. win), n_bins %u (1 .. min(256, win / 2)), n_mels %u (1 .. 128), "
                    "0 <= f_lo %g < f_hi %g <= audio_Fs %g / 2",
                    who, p->win, p->hop, p->n_bins, p->n_mels, p->f_lo, p->f_hi, p->audio_Fs);
    return FMRX_OK;
}

// one frame of the mono mix: its features
void frame_features(const float *m, const fmrx_audio_features_params &p, const audio_features::Tables &t, float *feat)
{
    const int win = static_cast<int>(p.win), n_bins = static_cast<int>(p.n_bins), n_mels = static_cast<int>(p.n_mels);
    float xw[kMaxWin], pw[audio_features::kMaxBins];
    for (int j = 0; j < win; j++) xw[j] = m[j] * t.w[j];
    for (int k = 0; k < n_bins; k++) {
        float re = 0.0f, im = 0.0f;
        int a = 0, b = win - win / 4;       // (k j) mod win and (k j - win/4) mod win
        for (int j = 0; j < win; j++) {
            re = fmaf(t.c[a], xw[j], re);
            im = fmaf(t.c[b], xw[j], im);
            a += k;
            if (a >= win) a -= win;
            b += k;
            if (b >= win) b -= win;
        }
        pw[k] = audio_features::bin_power(re, im);
    }
    for (int b = 0; b < n_mels; b++) feat[b] = audio_features::mel_chain(t.mel_w.data() + static_cast<size_t>(b) * n_bins, pw, t.lo[b], t.hi[b]);
}

int launch(fmrx_audio_features *m, const float *d_audio, size_t pitch, size_t n, hipStream_t s)
{
    AudioFeaturesArgs a;
    a.x = d_audio;
    a.pitch = pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->audio_channels;
    a.win = static_cast<int>(m->p.win);
    a.hop = static_cast<int>(m->p.hop);
    a.n_bins = static_cast<int>(m->p.n_bins);
    a.n_mels = static_cast<int>(m->p.n_mels);
    a.f_max = m->f_max;
    a.w = m->d_w.p;
    a.c = m->d_c.p;
    a.mel_w = m->d_mel_w.p;
    a.mel_lo = m->d_lo.p;
    a.mel_hi = m->d_hi.p;
    a.fill_in = m->d_fill[m->cur].p;
    a.carry_in = m->d_carry[m->cur].p;
    a.fill_out = m->d_fill[m->cur ^ 1].p;
    a.carry_out = m->d_carry[m->cur ^ 1].p;
    a.frames = m->d_frames.p;
    a.feat = m->d_feat.p;
    FMRX_TRY(audio_features_launch(a, s));
    m->cur ^= 1;
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_audio_features_preset(double audio_Fs, fmrx_audio_features_params *out)
{
    if (!out) return fail(FMRX_EINVAL, "audio_features_preset: null argument");
    fmrx_audio_features_params p = {};
    if (audio_Fs == 48000.0) {
        p.win = 1200;
        p.hop = 480;
    } else if (audio_Fs == 44100.0) {
        p.win = 1104;
        p.hop = 441;
    } else {
        return fail(FMRX_EINVAL, "audio_features_preset: audio_Fs %g: 48000 or 44100", audio_Fs);
    }
    p.n_bins = 201;
    p.n_mels = 80;
    p.f_lo = 0.0;
    p.f_hi = 8000.0;
    p.audio_Fs = audio_Fs;
    *out = p;
    return FMRX_OK;
}

int fmrx_audio_features_tables(const fmrx_audio_features_params *params, float *window, float *cosine, int32_t *mel_lo, int32_t *mel_hi, float *mel_w)
{
    FMRX_TRY(take_params("audio_features_tables", params));
    if (!window || !cosine || !mel_lo || !mel_hi || !mel_w) return fail(FMRX_EINVAL, "audio_features_tables: null argument");
    const audio_features::Tables t = audio_features::make_tables(*params);
    std::memcpy(window, t.w.data(), t.w.size() * sizeof(float));
    std::memcpy(cosine, t.c.data(), t.c.size() * sizeof(float));
    std::memcpy(mel_lo, t.lo.data(), t.lo.size() * sizeof(int32_t));
    std::memcpy(mel_hi, t.hi.data(), t.hi.size() * sizeof(int32_t));
    std::memcpy(mel_w, t.mel_w.data(), t.mel_w.size() * sizeof(float));
    return FMRX_OK;
}

size_t fmrx_audio_features_max_frames(const fmrx_audio_features_params *params, size_t n_audio)
{
    if (!audio_features::good_params(params) || n_audio < 1) return 0;
    return audio_features::max_frames(n_audio, params->hop);
}

int fmrx_audio_features_walk(const fmrx_audio_features_params *params, int audio_channels, const float *rows, size_t row_pitch, size_t n,
                             fmrx_audio_features_state *state_in_out, float *feat, uint32_t *frames)
{
    FMRX_TRY(take_params("audio_features_walk", params));
    if (!rows || !state_in_out || !feat || !frames) return fail(FMRX_EINVAL, "audio_features_walk: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "audio_features_walk: audio_channels must be 1 or 2");
    if (n < 1 || n > (size_t{1} << 26) || row_pitch < n) return fail(FMRX_EINVAL, "audio_features_walk: %zu samples (1 .. 2^26) in rows of %zu", n, row_pitch);
    const unsigned win = params->win, hop = params->hop, fill = state_in_out->fill;
    if (fill >= win) return fail(FMRX_EINVAL, "audio_features_walk: fill %u (0 .. %u)", fill, win - 1);
    const audio_features::Tables t = audio_features::make_tables(*params);
    // the stream: the carried mono mix, then the call's
    std::vector<float> e(fill + n);
    std::memcpy(e.data(), state_in_out->carry, fill * sizeof(float));
    for (size_t i = 0; i < n; i++) e[fill + i] = audio_channels == 2 ? audio_features::mono_mix(rows[i], rows[row_pitch + i]) : rows[i];
    const size_t F = audio_features::frames_of(static_cast<unsigned>(e.size()), win, hop), f_max = audio_features::max_frames(n, hop);
    std::memset(feat, 0, f_max * params->n_mels * sizeof(float));
    for (size_t q = 0; q < F; q++) frame_features(e.data() + q * hop, *params, t, feat + q * params->n_mels);
    const size_t left = e.size() - F * hop;
    std::memset(state_in_out->carry, 0, sizeof state_in_out->carry);
    std::memcpy(state_in_out->carry, e.data() + F * hop, left * sizeof(float));
    state_in_out->fill = static_cast<uint32_t>(left);
    *frames = static_cast<uint32_t>(F);
    return FMRX_OK;
}

int fmrx_audio_features_create(fmrx_audio_features **out, const fmrx_audio_features_params *params, int n_channels, int audio_channels, size_t n_audio,
                               int device)
{
    FMRX_TRY(take_params("audio_features_create", params));
    return meter_stage::create_on_audio("audio_features_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_audio_features *m) -> int {
        const size_t N = n_channels;
        m->p = *params;
        m->f_max = audio_features::max_frames(n_audio, params->hop);
        if (audio_features_tiles(N, m->f_max) > 0x7fffffffu)
            return fail(FMRX_EINVAL, "audio_features_create: %zu channels of %zu frames per call exceed a grid", N, m->f_max);
        const audio_features::Tables t = audio_features::make_tables(*params);
        const auto up = [](auto &buf, const auto &v) -> int {
            FMRX_TRY(buf.alloc(v.size()));
            FMRX_HIP(hipMemcpy(buf.p, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice));
            return FMRX_OK;
        };
        FMRX_TRY(up(m->d_w, t.w));
        FMRX_TRY(up(m->d_c, t.c));
        FMRX_TRY(up(m->d_mel_w, t.mel_w));
        FMRX_TRY(up(m->d_lo, t.lo));
        FMRX_TRY(up(m->d_hi, t.hi));
        for (int k = 0; k < 2; k++) {
            FMRX_TRY(m->d_fill[k].alloc(N));
            FMRX_TRY(m->d_carry[k].alloc(N * params->win));
            FMRX_HIP(hipMemset(m->d_fill[k].p, 0, m->d_fill[k].bytes()));
            FMRX_HIP(hipMemset(m->d_carry[k].p, 0, m->d_carry[k].bytes()));
        }
        FMRX_TRY(m->d_frames.alloc(N));
        FMRX_TRY(m->d_feat.alloc(N * m->f_max * params->n_mels));
        return FMRX_OK;
    });
}

int fmrx_audio_features_destroy(fmrx_audio_features *m) { return meter_stage::destroy(m); }

int fmrx_audio_features_reset(fmrx_audio_features *m, int channel)
{
    return meter_stage::reset_on_audio("audio_features_reset", m, channel, [&]() -> int {
        const DevBuf<unsigned> &f = m->d_fill[m->cur];
        const DevBuf<float> &c = m->d_carry[m->cur];
        const size_t per = m->p.win;
        if (channel < 0) {
            FMRX_HIP(hipMemset(f.p, 0, f.bytes()));
            FMRX_HIP(hipMemset(c.p, 0, c.bytes()));
        } else {
            FMRX_HIP(hipMemset(f.p + channel, 0, sizeof(unsigned)));
            FMRX_HIP(hipMemset(c.p + channel * per, 0, per * sizeof(float)));
        }
        return FMRX_OK;
    });
}

int fmrx_audio_features_state_get(fmrx_audio_features *m, fmrx_audio_features_state *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "audio_features_state_get: null argument");
    FMRX_TRY(m->wait());
    const size_t N = m->n_channels, win = m->p.win;
    std::vector<unsigned> fill(N);
    std::vector<float> carry(N * win);
    FMRX_HIP(hipMemcpy(fill.data(), m->d_fill[m->cur].p, N * sizeof(unsigned), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(carry.data(), m->d_carry[m->cur].p, carry.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::memset(out, 0, N * sizeof *out);
    for (size_t c = 0; c < N; c++) {
        out[c].fill = fill[c];
        std::memcpy(out[c].carry, carry.data() + c * win, (fill[c] < win ? fill[c] : win - 1) * sizeof(float));   // entries from fill on read 0
    }
    return FMRX_OK;
}

int fmrx_audio_features_process_dev(fmrx_audio_features *m, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    return meter_stage::read_dev("audio_features_process_dev", m, launch, d_audio, row_pitch, n, stream);
}

int fmrx_audio_features_result_dev(fmrx_audio_features *m, const float **d_feat, const uint32_t **d_frames)
{
    if (!m || !d_feat || !d_frames) return fail(FMRX_EINVAL, "audio_features_result_dev: null argument");
    *d_feat = m->d_feat.p;
    *d_frames = m->d_frames.p;
    return FMRX_OK;
}

int fmrx_audio_features_collect(fmrx_audio_features *m, float *feat, uint32_t *frames)
{
    FMRX_TRY(meter_stage::collected("audio_features_collect", m, feat));
    if (!frames) return fail(FMRX_EINVAL, "audio_features_collect: null argument");
    FMRX_HIP(hipMemcpy(feat, m->d_feat.p, m->d_feat.bytes(), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(frames, m->d_frames.p, m->d_frames.bytes(), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_audio_features_process(fmrx_audio_features *m, const float *audio, size_t row_pitch, size_t n, float *feat, uint32_t *frames)
{
    if (!frames) return fail(FMRX_EINVAL, "audio_features_process: null argument");
    return meter_stage::read_host("audio_features_process", m, launch, audio, row_pitch, n, feat, [&] { return fmrx_audio_features_collect(m, feat, frames); });
}

}  // extern "C"
