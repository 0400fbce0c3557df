// audio_meters.hip -- the audio meters' handle, host arithmetic and C ABI (include/fmrx.h: fmrx_audio_meters_*): per channel of a
// receiver bank and call, peak, sums, K-weighted energy, the stereo cross sum and the 100 ms bins of the audio rows.  Kernel:
// kernels_audio_meters.hip; one channel's walk, shared with fmrx_audio_meters_walk below: audio_meters_core.hpp; definition:
// tests/_audio_meters_model.py.
//
// A reader of meter_stage.hpp: it reads no meters and writes no audio.  Its own part is the channels' state on the device
// (field-major), the result arrays a call writes and their pinned host copies, the launch that fills them, the records' layout
// and the host arithmetic.
#include "audio_meters_core.hpp"
#include "meter_stage.hpp"

#include <cmath>

using namespace fmrx;
using meter_stage::field;

struct fmrx_audio_meters : meter_stage::Reader {
    double audio_Fs = 0.0;
    size_t bin_len = 0, max_bins = 0;
    audio_meters::Coefs coef;
    DevBuf<double> d_state, d_sums, d_bins;
    DevBuf<unsigned> d_fill, d_counts;
    HostBuf<double> h_sums, h_bins;
    HostBuf<unsigned> h_counts;
};

namespace {

bool good_fs(double Fs) { return std::isfinite(Fs) && Fs >= audio_meters::kMinFs && Fs <= audio_meters::kMaxFs; }

template <int AC>
void walk_channel(const audio_meters::Coefs &c, const float *rows, size_t pitch, size_t n, unsigned len, fmrx_audio_meter_state *st,
                  fmrx_audio_meter *rec, double *bins, size_t max_bins)
{
    audio_meters::Walk<AC> w;
    w.begin();
    for (int r = 0; r < AC; r++) {
        for (int i = 0; i < 4; i++) w.z[r][i] = st->z[r][i];
        w.bin_acc[r] = st->bin_acc[r];
    }
    w.bin_fill = static_cast<unsigned>(st->bin_fill);
    for (size_t k = 0; k < n; k++) {
        const float x[2] = {rows[k], rows[(AC - 1) * pitch + k]};
        w.sample(c, x, len, bins, max_bins);
    }
    w.finish(bins, max_bins);
    std::memset(rec, 0, sizeof *rec);
    rec->n = n;
    for (int r = 0; r < AC; r++) {
        for (int i = 0; i < 4; i++) st->z[r][i] = w.z[r][i];
        st->bin_acc[r] = w.bin_acc[r];
        rec->over[r] = w.over[r];
        rec->peak[r] = static_cast<double>(w.peak[r]);
        rec->sum_x[r] = w.sum_x[r];
        rec->sum_x2[r] = w.sum_x2[r];
        rec->sum_k2[r] = w.sum_k2[r];
    }
    st->bin_fill = w.bin_fill;
    rec->sum_lr = w.sum_lr;
    rec->bins_done = w.bins_done;
}

int launch(fmrx_audio_meters *m, const float *d_audio, size_t pitch, size_t n, hipStream_t s)
{
    AudioMetersArgs a;
    a.x = d_audio;
    a.pitch = pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->audio_channels;
    std::memcpy(a.coef, m->coef.q, sizeof a.coef);
    a.bin_len = static_cast<unsigned>(m->bin_len);
    a.max_bins = m->max_bins;
    a.state = m->d_state.p;
    a.fill = m->d_fill.p;
    a.sums = m->d_sums.p;
    a.counts = m->d_counts.p;
    a.bins = m->d_bins.p;
    FMRX_TRY(audio_meters_launch(a, s));
    FMRX_HIP(hipMemcpyAsync(m->h_sums.p, m->d_sums.p, m->d_sums.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipMemcpyAsync(m->h_counts.p, m->d_counts.p, m->d_counts.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipMemcpyAsync(m->h_bins.p, m->d_bins.p, m->d_bins.bytes(), hipMemcpyDeviceToHost, s));
    return FMRX_OK;
}

}  // namespace

namespace fmrx {
AudioMetersSums audio_meters_sums(const fmrx_audio_meters *m) { return AudioMetersSums{m->d_sums.p, m->n, m->n_channels, m->audio_channels, m->device, m->ran}; }
}  // namespace fmrx

extern "C" {

int fmrx_audio_meters_design(double audio_Fs, double *coef)
{
    if (!coef) return fail(FMRX_EINVAL, "audio_meters_design: null argument");
    if (!good_fs(audio_Fs)) return fail(FMRX_EINVAL, "audio_meters_design: audio_Fs %g (finite, %g .. %g)", audio_Fs, audio_meters::kMinFs, audio_meters::kMaxFs);
    audio_meters::Coefs c;
    audio_meters::design(audio_Fs, &c);
    std::memcpy(coef, c.q, sizeof c.q);
    return FMRX_OK;
}

size_t fmrx_audio_meters_bin_len(double audio_Fs) { return good_fs(audio_Fs) ? audio_meters::bin_len(audio_Fs) : 0; }

size_t fmrx_audio_meters_max_bins(double audio_Fs, size_t n_audio) { return good_fs(audio_Fs) ? n_audio / audio_meters::bin_len(audio_Fs) + 1 : 0; }

int fmrx_audio_meters_walk(double audio_Fs, int audio_channels, const float *rows, size_t row_pitch, size_t n, fmrx_audio_meter_state *state,
                           fmrx_audio_meter *rec, double *bins, size_t max_bins)
{
    if (!rows || !state || !rec || !bins) return fail(FMRX_EINVAL, "audio_meters_walk: null argument");
    if (!good_fs(audio_Fs)) return fail(FMRX_EINVAL, "audio_meters_walk: audio_Fs %g (finite, %g .. %g)", audio_Fs, audio_meters::kMinFs, audio_meters::kMaxFs);
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "audio_meters_walk: audio_channels must be 1 or 2");
    const size_t len = audio_meters::bin_len(audio_Fs);
    if (row_pitch < n || max_bins < n / len + 1) return fail(FMRX_EINVAL, "audio_meters_walk: a pitch shorter than its row, or %zu bins for %zu samples", max_bins, n);
    if (state->bin_fill >= len) return fail(FMRX_EINVAL, "audio_meters_walk: the state's bin_fill %llu is not below bin_len %zu", (unsigned long long)state->bin_fill, len);
    audio_meters::Coefs c;
    audio_meters::design(audio_Fs, &c);
    if (audio_channels == 2) {
        walk_channel<2>(c, rows, row_pitch, n, static_cast<unsigned>(len), state, rec, bins, max_bins);
    } else {
        walk_channel<1>(c, rows, row_pitch, n, static_cast<unsigned>(len), state, rec, bins, max_bins);
    }
    return FMRX_OK;
}

int fmrx_audio_meters_derive(const fmrx_audio_meter *m, int audio_channels, double full_scale, fmrx_audio_levels *out)
{
    FMRX_TRY(meter_stage::check_derive("audio_meters_derive", m, out, audio_channels, full_scale));
    const double n = static_cast<double>(m->n), fs2 = full_scale * full_scale;
    std::memset(out, 0, sizeof *out);
    for (int r = 0; r < 2; r++) {
        const bool has = r < audio_channels;
        out->peak_dbfs[r] = has ? db(m->peak[r] * m->peak[r], fs2) : -99.0;
        out->rms_dbfs[r] = has ? db(n > 0.0 ? m->sum_x2[r] / n : 0.0, fs2) : -99.0;
        out->dc[r] = has && n > 0.0 ? m->sum_x[r] / n : 0.0;
    }
    const double k2 = m->sum_k2[0] + (audio_channels == 2 ? m->sum_k2[1] : 0.0);
    out->loudness_lkfs = db(n > 0.0 ? k2 / n : 0.0, fs2, -0.691);
    if (audio_channels == 2) {
        const double den = std::sqrt(m->sum_x2[0] * m->sum_x2[1]);
        out->correlation = den > 0.0 && std::isfinite(den) ? m->sum_lr / den : 0.0;
        out->balance_db = db(m->sum_x2[0], m->sum_x2[1]);
    }
    out->over_fraction = meter_stage::over_fraction(m->over, m->n, audio_channels);
    return FMRX_OK;
}

int fmrx_audio_meters_create(fmrx_audio_meters **out, double audio_Fs, int n_channels, int audio_channels, size_t n_audio, int device)
{
    if (!good_fs(audio_Fs)) return fail(FMRX_EINVAL, "audio_meters_create: audio_Fs %g (finite, %g .. %g)", audio_Fs, audio_meters::kMinFs, audio_meters::kMaxFs);
    return meter_stage::create_on_audio("audio_meters_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_audio_meters *m) -> int {
        const size_t N = n_channels;
        m->audio_Fs = audio_Fs;
        m->bin_len = audio_meters::bin_len(audio_Fs);
        m->max_bins = n_audio / m->bin_len + 1;
        audio_meters::design(audio_Fs, &m->coef);
        FMRX_TRY(m->d_state.alloc(N * kAudioMetersStateFields));
        FMRX_TRY(m->d_fill.alloc(N));
        FMRX_TRY(m->d_sums.alloc(N * kAudioMetersSumFields));
        FMRX_TRY(m->d_counts.alloc(N * kAudioMetersCountFields));
        FMRX_TRY(m->d_bins.alloc(N * 2 * m->max_bins));
        FMRX_TRY(m->h_sums.alloc(m->d_sums.n));
        FMRX_TRY(m->h_counts.alloc(m->d_counts.n));
        FMRX_TRY(m->h_bins.alloc(m->d_bins.n));
        FMRX_TRY(meter_stage::clear_fields(m->d_state.p, kAudioMetersStateFields, n_channels, -1));
        return meter_stage::clear_fields(m->d_fill.p, 1, n_channels, -1);
    });
}

int fmrx_audio_meters_destroy(fmrx_audio_meters *m) { return meter_stage::destroy(m); }

int fmrx_audio_meters_reset(fmrx_audio_meters *m, int channel)
{
    return meter_stage::reset_on_audio("audio_meters_reset", m, channel, [&]() -> int {
        FMRX_TRY(meter_stage::clear_fields(m->d_state.p, kAudioMetersStateFields, m->n_channels, channel));
        return meter_stage::clear_fields(m->d_fill.p, 1, m->n_channels, channel);
    });
}

int fmrx_audio_meters_state_get(fmrx_audio_meters *m, fmrx_audio_meter_state *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "audio_meters_state_get: null argument");
    FMRX_TRY(m->wait());
    const int N = m->n_channels;
    std::vector<double> st(m->d_state.n);
    std::vector<unsigned> fill(m->d_fill.n);
    FMRX_HIP(hipMemcpy(st.data(), m->d_state.p, m->d_state.bytes(), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(fill.data(), m->d_fill.p, m->d_fill.bytes(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < static_cast<size_t>(N); c++) {
        for (int r = 0; r < 2; r++) {
            for (int i = 0; i < 4; i++) out[c].z[r][i] = field(st.data(), N, r * 4 + i, c);
            out[c].bin_acc[r] = field(st.data(), N, 8 + r, c);
        }
        out[c].bin_fill = fill[c];
    }
    return FMRX_OK;
}

int fmrx_audio_meters_process_dev(fmrx_audio_meters *m, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    return meter_stage::read_dev("audio_meters_process_dev", m, launch, d_audio, row_pitch, n, stream);
}

int fmrx_audio_meters_collect(fmrx_audio_meters *m, fmrx_audio_meter *out, double *bins)
{
    FMRX_TRY(meter_stage::collected("audio_meters_collect", m, out));
    const int N = m->n_channels;
    for (size_t c = 0; c < static_cast<size_t>(N); c++) {
        fmrx_audio_meter &r = out[c];
        r.n = m->n;
        for (int k = 0; k < 2; k++) {
            r.peak[k] = field(m->h_sums.p, N, 0 + k, c);
            r.sum_x[k] = field(m->h_sums.p, N, 2 + k, c);
            r.sum_x2[k] = field(m->h_sums.p, N, 4 + k, c);
            r.sum_k2[k] = field(m->h_sums.p, N, 6 + k, c);
            r.over[k] = field(m->h_counts.p, N, k, c);
        }
        r.sum_lr = field(m->h_sums.p, N, 8, c);
        r.bins_done = field(m->h_counts.p, N, 2, c);
    }
    if (bins) std::memcpy(bins, m->h_bins.p, m->h_bins.bytes());
    return FMRX_OK;
}

int fmrx_audio_meters_process(fmrx_audio_meters *m, const float *audio, size_t row_pitch, size_t n, fmrx_audio_meter *out, double *bins)
{
    return meter_stage::read_host("audio_meters_process", m, launch, audio, row_pitch, n, out, [&] { return fmrx_audio_meters_collect(m, out, bins); });
}

}  // extern "C"
