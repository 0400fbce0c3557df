// true_peak.hip -- the true-peak meter's handle, host arithmetic and C ABI (include/fmrx.h: fmrx_true_peak_*): per channel of a
// receiver bank and call, the peak of the 4x oversampled waveform, the sample peak and the groups beyond a limit.  Kernel:
// kernels_true_peak.hip; the interpolator, shared with fmrx_true_peak_walk below: true_peak_core.hpp; definition:
// tests/_true_peak_model.py.
//
// A handle of the audio meters' kind (audio_meters.hip): it only reads the rows.  It keeps the rows' carried samples on the
// device in two buffers, one read and one written per call (field-major, see fmrx_internal.hpp), the result array a call
// writes, its pinned host copy, and meter_stage.hpp's handle base: the event the last call recorded behind the copy; collect
// waits on that event, not on the device.
#include "meter_stage.hpp"
#include "true_peak_core.hpp"

#include <cmath>

using namespace fmrx;

struct fmrx_true_peak : meter_stage::Handle {
    int n_channels = 0, ac = 1;
    size_t n_audio = 0;
    float limit = 0.0f;
    DevBuf<float> d_state[2];
    int cur = 0;                 // the buffer the next call reads
    DevBuf<unsigned> d_res;
    unsigned *h_res = nullptr;   // pinned
    size_t n = 0;                // of the last call
    DevBuf<float> d_rows;        // fmrx_true_peak_process only
    ~fmrx_true_peak()
    {
        if (h_res) (void)hipHostFree(h_res);
    }
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
    if (!m || !out) return fail(FMRX_EINVAL, "true_peak_derive: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "true_peak_derive: audio_channels must be 1 or 2");
    if (!(full_scale > 0.0) || !std::isfinite(full_scale)) return fail(FMRX_EINVAL, "true_peak_derive: full_scale %g", full_scale);
    const double n = static_cast<double>(m->n), fs2 = full_scale * full_scale;
    std::memset(out, 0, sizeof *out);
    out->max_dbtp = -99.0;
    for (int r = 0; r < 2; r++) {
        const bool has = r < audio_channels;
        out->true_peak_dbtp[r] = has ? db(m->true_peak[r] * m->true_peak[r], fs2) : -99.0;
        out->peak_dbfs[r] = has ? db(m->peak[r] * m->peak[r], fs2) : -99.0;
        if (out->true_peak_dbtp[r] > out->max_dbtp) out->max_dbtp = out->true_peak_dbtp[r];
    }
    out->over_fraction = n > 0.0 ? (static_cast<double>(m->over[0]) + static_cast<double>(m->over[1])) / (n * audio_channels) : 0.0;
    return FMRX_OK;
}

int fmrx_true_peak_create(fmrx_true_peak **out, int n_channels, int audio_channels, size_t n_audio, float limit, int device)
{
    if (!out) return fail(FMRX_EINVAL, "true_peak_create: null argument");
    if (n_channels < 1) return fail(FMRX_EINVAL, "true_peak_create: n_channels must be >= 1");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "true_peak_create: audio_channels must be 1 or 2");
    if (n_audio < 1 || n_audio > (size_t{1} << 26)) return fail(FMRX_EINVAL, "true_peak_create: n_audio %zu (1 .. 2^26)", n_audio);
    if (!good_limit(limit)) return fail(FMRX_EINVAL, "true_peak_create: limit %g (finite, > 0)", limit);
    return meter_stage::make(out, device, [&](fmrx_true_peak *m) -> int {
        const size_t N = n_channels;
        m->n_channels = n_channels;
        m->ac = audio_channels;
        m->n_audio = n_audio;
        m->limit = limit;
        for (auto &b : m->d_state) {
            FMRX_TRY(b.alloc(N * kTruePeakStateFields));
            FMRX_HIP(hipMemset(b.p, 0, b.bytes()));
        }
        FMRX_TRY(m->d_res.alloc(N * kTruePeakFields));
        FMRX_HIP(hipHostMalloc(reinterpret_cast<void **>(&m->h_res), m->d_res.bytes(), hipHostMallocDefault));
        FMRX_HIP(hipStreamSynchronize(nullptr));
        return FMRX_OK;
    });
}

int fmrx_true_peak_destroy(fmrx_true_peak *m) { return meter_stage::destroy(m); }

int fmrx_true_peak_reset(fmrx_true_peak *m, int channel)
{
    if (!m) return fail(FMRX_EINVAL, "true_peak_reset: null handle");
    if (channel >= m->n_channels) return fail(FMRX_EINVAL, "true_peak_reset: channel %d of %d", channel, m->n_channels);
    FMRX_TRY(m->wait());
    DevBuf<float> &b = m->d_state[m->cur];
    if (channel < 0) FMRX_HIP(hipMemset(b.p, 0, b.bytes()));
    else FMRX_HIP(hipMemset2D(b.p + channel, m->n_channels * sizeof(float), 0, sizeof(float), kTruePeakStateFields));   // the channel's column
    FMRX_HIP(hipStreamSynchronize(nullptr));   // clear before this returns: a call on any stream, non-blocking ones included, finds it so
    return FMRX_OK;
}

int fmrx_true_peak_state_get(fmrx_true_peak *m, float *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "true_peak_state_get: null argument");
    FMRX_TRY(m->wait());
    const size_t N = m->n_channels;
    std::vector<float> st(N * kTruePeakStateFields);
    FMRX_HIP(hipMemcpy(st.data(), m->d_state[m->cur].p, st.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < N; c++)
        for (int f = 0; f < kTruePeakStateFields; f++) out[c * kTruePeakStateFields + f] = f < m->ac * kCarry ? st[f * N + c] : 0.0f;
    return FMRX_OK;
}

int fmrx_true_peak_process_dev(fmrx_true_peak *m, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    if (!m || !d_audio) return fail(FMRX_EINVAL, "true_peak_process_dev: null argument");
    if (n < 1 || n > m->n_audio) return fail(FMRX_EINVAL, "true_peak_process_dev: %zu samples per row (1 .. the handle's n_audio %zu)", n, m->n_audio);
    if (row_pitch < n) return fail(FMRX_EINVAL, "true_peak_process_dev: pitch of %zu floats is shorter than a row's %zu samples", row_pitch, n);
    FMRX_HIP(hipSetDevice(m->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TruePeakArgs a;
    a.x = d_audio;
    a.pitch = row_pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->ac;
    a.limit = m->limit;
    a.state_in = m->d_state[m->cur].p;
    a.state_out = m->d_state[m->cur ^ 1].p;
    a.res = m->d_res.p;
    FMRX_TRY(true_peak_launch(a, s));
    m->cur ^= 1;
    FMRX_HIP(hipMemcpyAsync(m->h_res, m->d_res.p, m->d_res.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipEventRecord(m->done, s));
    m->n = n;
    m->ran = true;
    return FMRX_OK;
}

int fmrx_true_peak_collect(fmrx_true_peak *m, fmrx_true_peak_record *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "true_peak_collect: null argument");
    if (!m->ran) return fail(FMRX_EINVAL, "true_peak_collect: no call to collect");
    FMRX_TRY(m->wait());
    const size_t N = m->n_channels;
    for (size_t c = 0; c < N; c++) {
        fmrx_true_peak_record &r = out[c];
        r.n = m->n;
        for (int k = 0; k < 2; k++) {
            r.true_peak[k] = static_cast<double>(bits_float(m->h_res[(0 + k) * N + c]));
            r.peak[k] = static_cast<double>(bits_float(m->h_res[(2 + k) * N + c]));
            r.over[k] = m->h_res[(4 + k) * N + c];
        }
    }
    return FMRX_OK;
}

int fmrx_true_peak_process(fmrx_true_peak *m, const float *audio, size_t row_pitch, size_t n, fmrx_true_peak_record *out)
{
    if (!m || !audio || !out) return fail(FMRX_EINVAL, "true_peak_process: null argument");
    if (n < 1 || n > m->n_audio) return fail(FMRX_EINVAL, "true_peak_process: %zu samples per row (1 .. the handle's n_audio %zu)", n, m->n_audio);
    if (row_pitch < n) return fail(FMRX_EINVAL, "true_peak_process: a pitch shorter than its row");
    FMRX_TRY(m->wait());   // this call runs on the null stream
    const size_t rows = static_cast<size_t>(m->n_channels) * m->ac, dp = (n + 3) / 4 * 4;   // the device copy's rows are 16-byte aligned
    FMRX_TRY(m->d_rows.ensure(dp * rows));
    FMRX_HIP(hipMemcpy2D(m->d_rows.p, dp * sizeof(float), audio, row_pitch * sizeof(float), n * sizeof(float), rows, hipMemcpyHostToDevice));
    FMRX_TRY(fmrx_true_peak_process_dev(m, m->d_rows.p, dp, n, nullptr));
    return fmrx_true_peak_collect(m, out);
}

}  // extern "C"
