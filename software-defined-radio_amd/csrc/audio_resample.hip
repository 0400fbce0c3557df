// audio_resample.hip -- the audio rate converter's handle, host arithmetic and C ABI (include/fmrx.h: fmrx_audio_resample_*): per
// channel of a receiver bank, the channel's mono mix or each of its rows through a polyphase FIR at a rational rate up / down,
// history and phase carried from call to call, left on the device as [n_channels][R][M_max] float32 and / or s16.  Kernel:
// kernels_audio_resample.hip; the taps, the positions and the chains, shared with fmrx_audio_resample_walk below:
// audio_resample_core.hpp; definition: tests/_audio_resample_model.py.
//
// A reader of meter_stage.hpp: it only reads the rows.  Its own part is the geometry and its tap table on the device, the carried
// state on the device in two pairs of buffers, one read and one written per call (channel-major: pos, and taps - 1 floats per
// converted row), the results a call writes (the rows and the counts, which stay on the device until a collect asks for them) and
// the host arithmetic.
#include "meter_stage.hpp"
#include "audio_resample_core.hpp"

#include <cmath>

using namespace fmrx;

struct fmrx_audio_resample : meter_stage::Reader {
    fmrx_audio_resample_params p = {};
    int rows_out = 1;            // R
    size_t m_max = 0;
    unsigned tile_out = 0;
    int wrap = 1;                // of the call being launched
    DevBuf<float> d_h;
    DevBuf<unsigned> d_pos[2];
    DevBuf<float> d_carry[2];    // [n_channels][R][taps - 1]
    int cur = 0;                 // the buffers the next call reads
    DevBuf<unsigned> d_counts;
    DevBuf<float> d_f32;         // [n_channels][R][m_max], where the handle keeps it
    DevBuf<int16_t> d_pcm;
    bool want_f32 = false, want_pcm = false;
};

namespace {

static_assert(sizeof(fmrx_audio_resample_state::carry) == 2 * audio_resample::kMaxCarry * sizeof(float), "a row's carry holds taps - 1 samples at most");

int take_params(const char *who, const fmrx_audio_resample_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (!audio_resample::good_params(p))
        return fail(FMRX_EINVAL,
                    "%s: up %u (1 .. 160), down %u (1 .. 1024, coprime to up), taps %u (a multiple of 4, 8 .. 256, up taps <= 16384), mix %u (0, 1), "
                    "cutoff %g (0 < .. <= 1), beta %g (0 .. 20)",
                    who, p->up, p->down, p->taps, p->mix, p->cutoff, p->beta);
    return FMRX_OK;
}

int take_policy(const char *who, int pcm_policy)
{
    if (pcm_policy != FMRX_PCM_WRAP && pcm_policy != FMRX_PCM_SATURATE) return fail(FMRX_EINVAL, "%s: pcm_policy %d", who, pcm_policy);
    return FMRX_OK;
}

int launch(fmrx_audio_resample *m, const float *d_audio, size_t pitch, size_t n, hipStream_t s)
{
    AudioResampleArgs a;
    a.x = d_audio;
    a.pitch = pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->audio_channels;
    a.rows = m->rows_out;
    a.up = m->p.up;
    a.down = m->p.down;
    a.taps = m->p.taps;
    a.h = m->d_h.p;
    a.pos_in = m->d_pos[m->cur].p;
    a.carry_in = m->d_carry[m->cur].p;
    a.pos_out = m->d_pos[m->cur ^ 1].p;
    a.carry_out = m->d_carry[m->cur ^ 1].p;
    a.m_max = m->m_max;
    a.tile_out = m->tile_out;
    a.out_f32 = m->want_f32 ? m->d_f32.p : nullptr;
    a.out_pcm = m->want_pcm ? m->d_pcm.p : nullptr;
    a.wrap = m->wrap;
    a.counts = m->d_counts.p;
    FMRX_TRY(audio_resample_launch(a, s));
    m->cur ^= 1;
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_audio_resample_preset(double audio_Fs, double out_Fs, int mix, fmrx_audio_resample_params *out)
{
    if (!out) return fail(FMRX_EINVAL, "audio_resample_preset: null argument");
    const auto rate = [](double f) { return f >= 8000.0 && f <= 48000.0 && f == std::floor(f); };   // false for a NaN
    if (!rate(audio_Fs) || !rate(out_Fs)) return fail(FMRX_EINVAL, "audio_resample_preset: rates %g -> %g: integers within 8000 .. 48000", audio_Fs, out_Fs);
    if (mix != 0 && mix != 1) return fail(FMRX_EINVAL, "audio_resample_preset: mix %d", mix);
    const unsigned fi = static_cast<unsigned>(audio_Fs), fo = static_cast<unsigned>(out_Fs), g = audio_resample::gcd(fo, fi);
    fmrx_audio_resample_params p = {};
    p.up = fo / g;
    p.down = fi / g;
    // 4 ceil(24 / min(1, up / down) / 4) in integers: 24 down / up, rounded up to a multiple of 4
    p.taps = p.up >= p.down ? 24u : static_cast<unsigned>((24ull * p.down + 4ull * p.up - 1) / (4ull * p.up)) * 4u;
    p.mix = static_cast<uint32_t>(mix);
    p.cutoff = 0.9;
    p.beta = 8.0;
    if (!audio_resample::good_params(&p))
        return fail(FMRX_EINVAL, "audio_resample_preset: %g -> %g is %u/%u with %u taps: beyond the limits", audio_Fs, out_Fs, p.up, p.down, p.taps);
    *out = p;
    return FMRX_OK;
}

int fmrx_audio_resample_taps(const fmrx_audio_resample_params *params, float *h)
{
    FMRX_TRY(take_params("audio_resample_taps", params));
    if (!h) return fail(FMRX_EINVAL, "audio_resample_taps: null argument");
    const std::vector<float> t = audio_resample::make_taps(*params);
    std::memcpy(h, t.data(), t.size() * sizeof(float));
    return FMRX_OK;
}

size_t fmrx_audio_resample_max_out(const fmrx_audio_resample_params *params, size_t n_audio)
{
    if (!audio_resample::good_params(params) || n_audio < 1 || n_audio > (size_t{1} << 26)) return 0;
    return audio_resample::max_out(n_audio, params->up, params->down);
}

double fmrx_audio_resample_latency(const fmrx_audio_resample_params *params)
{
    if (!audio_resample::good_params(params)) return std::nan("");
    return (static_cast<double>(params->up) * params->taps - 1.0) / (2.0 * params->up);
}

int fmrx_audio_resample_walk(const fmrx_audio_resample_params *params, int audio_channels, const float *rows, size_t row_pitch, size_t n,
                             fmrx_audio_resample_state *state_in_out, float *out, uint32_t *count)
{
    FMRX_TRY(take_params("audio_resample_walk", params));
    if (!rows || !state_in_out || !out || !count) return fail(FMRX_EINVAL, "audio_resample_walk: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "audio_resample_walk: audio_channels must be 1 or 2");
    if (n < 1 || n > (size_t{1} << 26) || row_pitch < n) return fail(FMRX_EINVAL, "audio_resample_walk: %zu samples (1 .. 2^26) in rows of %zu", n, row_pitch);
    const unsigned U = params->up, D = params->down, T = params->taps, pos = state_in_out->pos;
    if (pos >= D) return fail(FMRX_EINVAL, "audio_resample_walk: pos %u (0 .. %u)", pos, D - 1);
    const int R = audio_resample::rows_of(*params, audio_channels);
    const size_t C = T - 1, m_max = audio_resample::max_out(n, U, D);
    const uint64_t M = audio_resample::outputs_of(n, U, D, pos);
    const std::vector<float> h = audio_resample::make_taps(*params);
    std::memset(out, 0, static_cast<size_t>(R) * m_max * sizeof(float));
    std::vector<float> e(C + n);
    for (int r = 0; r < R; r++) {
        // the stream: the carried samples, then the call's
        std::memcpy(e.data(), state_in_out->carry[r], C * sizeof(float));
        const float *row = rows + r * row_pitch;
        for (size_t i = 0; i < n; i++) e[C + i] = params->mix && audio_channels == 2 ? audio_resample::mono_mix(row[i], row[row_pitch + i]) : row[i];
        for (uint64_t q = 0; q < M; q++) {
            const uint64_t t = pos + q * D;
            out[r * m_max + q] = audio_resample::chain(h.data() + (t % U) * T, e.data() + C + t / U, static_cast<int>(T));
        }
        std::memset(state_in_out->carry[r], 0, sizeof state_in_out->carry[r]);
        std::memcpy(state_in_out->carry[r], e.data() + n, C * sizeof(float));
    }
    state_in_out->pos = static_cast<uint32_t>(pos + M * D - static_cast<uint64_t>(n) * U);
    *count = static_cast<uint32_t>(M);
    return FMRX_OK;
}

int fmrx_audio_resample_create(fmrx_audio_resample **out, const fmrx_audio_resample_params *params, int n_channels, int audio_channels, size_t n_audio,
                               int want_f32, int want_pcm, int device)
{
    FMRX_TRY(take_params("audio_resample_create", params));
    if (!want_f32 && !want_pcm) return fail(FMRX_EINVAL, "audio_resample_create: neither float nor PCM results");
    return meter_stage::create_on_audio("audio_resample_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_audio_resample *m) -> int {
        const size_t N = n_channels;
        m->p = *params;
        m->rows_out = audio_resample::rows_of(*params, audio_channels);
        m->m_max = audio_resample::max_out(n_audio, params->up, params->down);
        m->tile_out = audio_resample_tile_out(params->up, params->down, params->taps);
        m->want_f32 = want_f32 != 0;
        m->want_pcm = want_pcm != 0;
        const size_t tiles = (m->m_max + m->tile_out - 1) / m->tile_out;
        if (tiles > 65535) return fail(FMRX_EINVAL, "audio_resample_create: %zu outputs per row in tiles of %u exceed a grid", m->m_max, m->tile_out);
        const std::vector<float> h = audio_resample::make_taps(*params);
        FMRX_TRY(m->d_h.alloc(h.size()));
        FMRX_HIP(hipMemcpy(m->d_h.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        for (int k = 0; k < 2; k++) {
            FMRX_TRY(m->d_pos[k].alloc(N));
            FMRX_TRY(m->d_carry[k].alloc(N * m->rows_out * (params->taps - 1)));
            FMRX_HIP(hipMemset(m->d_pos[k].p, 0, m->d_pos[k].bytes()));
            FMRX_HIP(hipMemset(m->d_carry[k].p, 0, m->d_carry[k].bytes()));
        }
        FMRX_TRY(m->d_counts.alloc(N));
        FMRX_HIP(hipMemset(m->d_counts.p, 0, m->d_counts.bytes()));
        const size_t total = N * m->rows_out * m->m_max;
        if (m->want_f32) {
            FMRX_TRY(m->d_f32.alloc(total));
            FMRX_HIP(hipMemset(m->d_f32.p, 0, m->d_f32.bytes()));
        }
        if (m->want_pcm) {
            FMRX_TRY(m->d_pcm.alloc(total));
            FMRX_HIP(hipMemset(m->d_pcm.p, 0, m->d_pcm.bytes()));
        }
        return FMRX_OK;
    });
}

int fmrx_audio_resample_destroy(fmrx_audio_resample *m) { return meter_stage::destroy(m); }

int fmrx_audio_resample_reset(fmrx_audio_resample *m, int channel)
{
    return meter_stage::reset_on_audio("audio_resample_reset", m, channel, [&]() -> int {
        const DevBuf<unsigned> &f = m->d_pos[m->cur];
        const DevBuf<float> &c = m->d_carry[m->cur];
        const size_t per = static_cast<size_t>(m->rows_out) * (m->p.taps - 1);
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

int fmrx_audio_resample_state_get(fmrx_audio_resample *m, fmrx_audio_resample_state *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "audio_resample_state_get: null argument");
    FMRX_TRY(m->wait());
    const size_t N = m->n_channels, C = m->p.taps - 1, R = m->rows_out;
    std::vector<unsigned> pos(N);
    std::vector<float> carry(N * R * C);
    FMRX_HIP(hipMemcpy(pos.data(), m->d_pos[m->cur].p, N * sizeof(unsigned), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(carry.data(), m->d_carry[m->cur].p, carry.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::memset(out, 0, N * sizeof *out);
    for (size_t c = 0; c < N; c++) {
        out[c].pos = pos[c];
        for (size_t r = 0; r < R; r++) std::memcpy(out[c].carry[r], carry.data() + (c * R + r) * C, C * sizeof(float));
    }
    return FMRX_OK;
}

int fmrx_audio_resample_process_dev(fmrx_audio_resample *m, const float *d_audio, size_t row_pitch, size_t n, int pcm_policy, void *stream)
{
    FMRX_TRY(meter_stage::check_read("audio_resample_process_dev", m, d_audio, row_pitch, n));
    FMRX_TRY(take_policy("audio_resample_process_dev", pcm_policy));
    m->wrap = pcm_policy == FMRX_PCM_WRAP ? 1 : 0;
    return meter_stage::read_dev("audio_resample_process_dev", m, launch, d_audio, row_pitch, n, stream);
}

int fmrx_audio_resample_result_dev(fmrx_audio_resample *m, const float **d_f32, const int16_t **d_pcm, const uint32_t **d_counts)
{
    if (!m || !d_f32 || !d_pcm || !d_counts) return fail(FMRX_EINVAL, "audio_resample_result_dev: null argument");
    *d_f32 = m->want_f32 ? m->d_f32.p : nullptr;
    *d_pcm = m->want_pcm ? m->d_pcm.p : nullptr;
    *d_counts = m->d_counts.p;
    return FMRX_OK;
}

int fmrx_audio_resample_collect(fmrx_audio_resample *m, float *out_f32, int16_t *out_pcm, uint32_t *counts)
{
    FMRX_TRY(meter_stage::collected("audio_resample_collect", m, counts));
    if ((out_f32 && !m->want_f32) || (out_pcm && !m->want_pcm)) return fail(FMRX_EINVAL, "audio_resample_collect: the handle does not keep that result");
    if (out_f32) FMRX_HIP(hipMemcpy(out_f32, m->d_f32.p, m->d_f32.bytes(), hipMemcpyDeviceToHost));
    if (out_pcm) FMRX_HIP(hipMemcpy(out_pcm, m->d_pcm.p, m->d_pcm.bytes(), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(counts, m->d_counts.p, m->d_counts.bytes(), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_audio_resample_process(fmrx_audio_resample *m, const float *audio, size_t row_pitch, size_t n, int pcm_policy, float *out_f32, int16_t *out_pcm,
                                uint32_t *counts)
{
    FMRX_TRY(meter_stage::check_read("audio_resample_process", m, audio, row_pitch, n));
    FMRX_TRY(take_policy("audio_resample_process", pcm_policy));
    if ((out_f32 && !m->want_f32) || (out_pcm && !m->want_pcm)) return fail(FMRX_EINVAL, "audio_resample_process: the handle does not keep that result");
    FMRX_TRY(m->wait());   // the policy is the handle's until the launch
    m->wrap = pcm_policy == FMRX_PCM_WRAP ? 1 : 0;
    return meter_stage::read_host("audio_resample_process", m, launch, audio, row_pitch, n, counts, [&] { return fmrx_audio_resample_collect(m, out_f32, out_pcm, counts); });
}

}  // extern "C"
