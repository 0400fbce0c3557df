// true_peak.hip -- the true-peak meter's handle, host arithmetic and C ABI (include/fmrx.h: fmrx_true_peak_*): per channel of a
// receiver bank and call, the peak of the 4x oversampled waveform, the sample peak and the groups beyond a limit.  Kernel:
// kernels_true_peak.hip; the interpolator, shared with fmrx_true_peak_walk below: true_peak_core.hpp; definition:
// tests/_true_peak_model.py.
//
// A reader of meter_stage.hpp: it only reads the rows.  Its own part is the rows' carried samples on the device in two buffers,
// one read and one written per call (field-major), the result array a call writes and its pinned host copy, the launch that
// fills them, the records' layout and the host arithmetic.
#include "meter_stage.hpp"
#include "true_peak_core.hpp"

#include <cmath>

using namespace fmrx;
using meter_stage::field;

struct fmrx_true_peak : meter_stage::Reader {
    float limit = 0.0f;
    DevBuf<float> d_state[2];
    int cur = 0;                 // the buffer the next call reads
    DevBuf<unsigned> d_res;
    HostBuf<unsigned> h_res;
};

namespace {

constexpr int kCarry = true_peak::kCarry, kRun = true_peak::kRun;

bool good_limit(float limit) { return limit > 0.0f && limit - limit == 0.0f; }

float bits_float(unsigned u)
{
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}

// one row of one channel: the stream is the carried samples, then the row; sample i of the call closes the group that reads
// the stream's entries i .. i + 11
void walk_row(const float *row, size_t n, float limit, float *carry, true_peak::Row &acc)
{
    std::vector<float> e(kCarry + n + kRun);   // zeros behind the row, for the last run's groups that do not count
    std::memcpy(e.data(), carry, kCarry * sizeof(float));
    std::memcpy(e.data() + kCarry, row, n * sizeof(float));
    for (size_t i = 0; i < n; i += kRun) {
        float w[kRun + kCarry];
        std::memcpy(w, e.data() + i, sizeof w);
        true_peak::run<kRun>(w, n - i < static_cast<size_t>(kRun) ? static_cast<int>(n - i) : kRun, limit, acc);
    }
    std::memcpy(carry, e.data() + n, kCarry * sizeof(float));
}

int launch(fmrx_true_peak *m, const float *d_audio, size_t pitch, size_t n, hipStream_t s)
{
    TruePeakArgs a;
    a.x = d_audio;
    a.pitch = pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->audio_channels;
    a.limit = m->limit;
    a.state_in = m->d_state[m->cur].p;
    a.state_out = m->d_state[m->cur ^ 1].p;
    a.res = m->d_res.p;
    FMRX_TRY(true_peak_launch(a, s));
    m->cur ^= 1;
    FMRX_HIP(hipMemcpyAsync(m->h_res.p, m->d_res.p, m->d_res.bytes(), hipMemcpyDeviceToHost, s));
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_true_peak_taps(float *h36)
{
    if (!h36) return fail(FMRX_EINVAL, "true_peak_taps: null argument");
    const float h[3 * true_peak::kTaps] = {FMRX_TP_H1, FMRX_TP_H2, FMRX_TP_H3};
    std::memcpy(h36, h, sizeof h);
    return FMRX_OK;
}

size_t fmrx_true_peak_latency(void) { return true_peak::kLatency; }

size_t fmrx_true_peak_tile(void) { return true_peak::kTile; }

int fmrx_true_peak_walk(int audio_channels, const float *rows, size_t row_pitch, size_t n, float limit, float *state_in_out, fmrx_true_peak_record *rec)
{
    if (!rows || !state_in_out || !rec) return fail(FMRX_EINVAL, "true_peak_walk: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "true_peak_walk: audio_channels must be 1 or 2");
    if (n < 1 || n > (size_t{1} << 26) || row_pitch < n) return fail(FMRX_EINVAL, "true_peak_walk: %zu samples (1 .. 2^26) in rows of %zu", n, row_pitch);
    if (!good_limit(limit)) return fail(FMRX_EINVAL, "true_peak_walk: limit %g (finite, > 0)", limit);
    std::memset(rec, 0, sizeof *rec);
    rec->n = n;
    for (int r = 0; r < audio_channels; r++) {
        true_peak::Row acc;
        walk_row(rows + r * row_pitch, n, limit, state_in_out + r * kCarry, acc);
        rec->over[r] = acc.over;
        rec->true_peak[r] = static_cast<double>(acc.tp);
        rec->peak[r] = static_cast<double>(acc.pk);
    }
    return FMRX_OK;
}

int fmrx_true_peak_derive(const fmrx_true_peak_record *m, int audio_channels, double full_scale, fmrx_true_peak_levels *out)
{
    FMRX_TRY(meter_stage::check_derive("true_peak_derive", m, out, audio_channels, full_scale));
    const double fs2 = full_scale * full_scale;
    std::memset(out, 0, sizeof *out);
    out->max_dbtp = -99.0;
    for (int r = 0; r < 2; r++) {
        const bool has = r < audio_channels;
        out->true_peak_dbtp[r] = has ? db(m->true_peak[r] * m->true_peak[r], fs2) : -99.0;
        out->peak_dbfs[r] = has ? db(m->peak[r] * m->peak[r], fs2) : -99.0;
        if (out->true_peak_dbtp[r] > out->max_dbtp) out->max_dbtp = out->true_peak_dbtp[r];
    }
    out->over_fraction = meter_stage::over_fraction(m->over, m->n, audio_channels);
    return FMRX_OK;
}

int fmrx_true_peak_create(fmrx_true_peak **out, int n_channels, int audio_channels, size_t n_audio, float limit, int device)
{
    if (!good_limit(limit)) return fail(FMRX_EINVAL, "true_peak_create: limit %g (finite, > 0)", limit);
    return meter_stage::create_on_audio("true_peak_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_true_peak *m) -> int {
        const size_t N = n_channels;
        m->limit = limit;
        for (auto &b : m->d_state) {
            FMRX_TRY(b.alloc(N * kTruePeakStateFields));
            FMRX_TRY(meter_stage::clear_fields(b.p, kTruePeakStateFields, n_channels, -1));
        }
        FMRX_TRY(m->d_res.alloc(N * kTruePeakFields));
        return m->h_res.alloc(m->d_res.n);
    });
}

int fmrx_true_peak_destroy(fmrx_true_peak *m) { return meter_stage::destroy(m); }

int fmrx_true_peak_reset(fmrx_true_peak *m, int channel)
{
    return meter_stage::reset_on_audio("true_peak_reset", m, channel,
                                       [&] { return meter_stage::clear_fields(m->d_state[m->cur].p, kTruePeakStateFields, m->n_channels, channel); });
}

int fmrx_true_peak_state_get(fmrx_true_peak *m, float *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "true_peak_state_get: null argument");
    FMRX_TRY(m->wait());
    const DevBuf<float> &b = m->d_state[m->cur];
    std::vector<float> st(b.n);
    FMRX_HIP(hipMemcpy(st.data(), b.p, b.bytes(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < static_cast<size_t>(m->n_channels); c++)
        for (int f = 0; f < kTruePeakStateFields; f++)
            out[c * kTruePeakStateFields + f] = f < m->audio_channels * kCarry ? field(st.data(), m->n_channels, f, c) : 0.0f;
    return FMRX_OK;
}

int fmrx_true_peak_process_dev(fmrx_true_peak *m, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    return meter_stage::read_dev("true_peak_process_dev", m, launch, d_audio, row_pitch, n, stream);
}

int fmrx_true_peak_collect(fmrx_true_peak *m, fmrx_true_peak_record *out)
{
    FMRX_TRY(meter_stage::collected("true_peak_collect", m, out));
    const int N = m->n_channels;
    for (size_t c = 0; c < static_cast<size_t>(N); c++) {
        fmrx_true_peak_record &r = out[c];
        r.n = m->n;
        for (int k = 0; k < 2; k++) {
            r.true_peak[k] = static_cast<double>(bits_float(field(m->h_res.p, N, 0 + k, c)));
            r.peak[k] = static_cast<double>(bits_float(field(m->h_res.p, N, 2 + k, c)));
            r.over[k] = field(m->h_res.p, N, 4 + k, c);
        }
    }
    return FMRX_OK;
}

int fmrx_true_peak_process(fmrx_true_peak *m, const float *audio, size_t row_pitch, size_t n, fmrx_true_peak_record *out)
{
    return meter_stage::read_host("true_peak_process", m, launch, audio, row_pitch, n, out, [&] { return fmrx_true_peak_collect(m, out); });
}

}  // extern "C"
