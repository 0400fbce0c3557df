// audio_spectrum.hip -- the audio spectrum meter's handle, host arithmetic and C ABI (include/fmrx.h: fmrx_audio_spectrum_*): per
// channel of a receiver bank and call, the power in up to 32 frequency bands of each audio row, summed over the 256-sample frames
// the call completed.  Kernels: kernels_audio_spectrum.hip; the tables and the frame arithmetic, shared with
// fmrx_audio_spectrum_walk below: audio_spectrum_core.hpp; definition: tests/_audio_spectrum_model.py.
//
// A reader of meter_stage.hpp: it only reads the rows.  Its own part is the carried state on the device in two pairs of buffers,
// one read and one written per call (channel-major: a row's open frame is 1 KiB that a workgroup reads in one piece), the band
// edges, the results a call writes (field-major [audio_channels n_bands][n_channels] doubles and the frames per channel) with
// their pinned host copies, the tile sums of rows too long for one tile, the records' layout and the host arithmetic.
#include "meter_stage.hpp"
#include "audio_spectrum_core.hpp"

#include <cmath>

using namespace fmrx;
using meter_stage::field;

struct fmrx_audio_spectrum : meter_stage::Reader {
    int n_bands = 0;
    int edges[audio_spectrum::kMaxBands + 1] = {};
    DevBuf<int> d_edges;
    DevBuf<unsigned> d_fill[2];
    DevBuf<float> d_carry[2];    // [n_channels][audio_channels][256]
    int cur = 0;                 // the buffers the next call reads
    DevBuf<unsigned> d_frames;
    HostBuf<unsigned> h_frames;
    DevBuf<double> d_res, d_tiles;
    HostBuf<double> h_res;
};

namespace {

constexpr int kFrame = audio_spectrum::kFrame, kBins = audio_spectrum::kBins, kTile = audio_spectrum::kTile, kMaxBands = audio_spectrum::kMaxBands;
constexpr audio_spectrum::Tables kTables = audio_spectrum::make_tables();

// edges == NULL: the default bands
int take_edges(const char *who, const int *edges, int n_bands, int *out, int *n_out)
{
    if (!edges) {
        edges = audio_spectrum::kDefaultEdges;
        n_bands = audio_spectrum::kDefaultBands;
    }
    if (!audio_spectrum::good_edges(edges, n_bands))
        return fail(FMRX_EINVAL, "%s: %d bands (1 .. 32) whose edges must ascend strictly within 1 .. 128", who, n_bands);
    std::memcpy(out, edges, (n_bands + 1) * sizeof(int));
    *n_out = n_bands;
    return FMRX_OK;
}

// one frame of one row: its band powers
void frame_bands(const float *x, const int *edges, int n_bands, float *bands)
{
    float xw[kFrame], p[kBins];
    for (int j = 0; j < kFrame; j++) xw[j] = x[j] * kTables.w[j];
    for (int k = 0; k < kBins; k++) {
        float re = 0.0f, im = 0.0f;
        for (int j = 0; j < kFrame; j++) {
            re = fmaf(kTables.c[(k * j) & (kFrame - 1)], xw[j], re);
            im = fmaf(kTables.c[(k * j - kFrame / 4) & (kFrame - 1)], xw[j], im);
        }
        p[k] = audio_spectrum::bin_power(re, im);
    }
    for (int b = 0; b < n_bands; b++) bands[b] = audio_spectrum::band_sum(p, edges[b], edges[b + 1]);
}

// one row of one channel: the stream is the open frame's `fill` samples, then the row; -> the call's two-level sums, and the
// samples behind the last completed frame in `carry`
void walk_row(const float *row, size_t n, const int *edges, int n_bands, unsigned fill, float *carry, double *band)
{
    std::vector<float> e(fill + n);
    std::memcpy(e.data(), carry, fill * sizeof(float));
    std::memcpy(e.data() + fill, row, n * sizeof(float));
    const size_t F = e.size() / kFrame, left = e.size() % kFrame;
    for (int b = 0; b < n_bands; b++) band[b] = 0.0;
    for (size_t t0 = 0; t0 < F; t0 += kTile) {
        double tile[kMaxBands] = {};
        for (size_t q = t0; q < F && q < t0 + kTile; q++) {
            float bp[kMaxBands];
            frame_bands(e.data() + q * kFrame, edges, n_bands, bp);
            for (int b = 0; b < n_bands; b++) tile[b] = tile[b] + static_cast<double>(bp[b]);
        }
        for (int b = 0; b < n_bands; b++) band[b] = band[b] + tile[b];
    }
    std::memset(carry, 0, (kFrame - 1) * sizeof(float));
    std::memcpy(carry, e.data() + F * kFrame, left * sizeof(float));
}

int launch(fmrx_audio_spectrum *m, const float *d_audio, size_t pitch, size_t n, hipStream_t s)
{
    AudioSpectrumArgs a;
    a.x = d_audio;
    a.pitch = pitch;
    a.n = n;
    a.n_channels = m->n_channels;
    a.ac = m->audio_channels;
    a.n_bands = m->n_bands;
    a.edges = m->d_edges.p;
    a.fill_in = m->d_fill[m->cur].p;
    a.carry_in = m->d_carry[m->cur].p;
    a.fill_out = m->d_fill[m->cur ^ 1].p;
    a.carry_out = m->d_carry[m->cur ^ 1].p;
    a.frames = m->d_frames.p;
    a.res = m->d_res.p;
    a.tiles = m->d_tiles.p;
    FMRX_TRY(audio_spectrum_launch(a, s));
    m->cur ^= 1;
    FMRX_HIP(hipMemcpyAsync(m->h_res.p, m->d_res.p, m->d_res.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipMemcpyAsync(m->h_frames.p, m->d_frames.p, m->d_frames.bytes(), hipMemcpyDeviceToHost, s));
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_audio_spectrum_tables(float *window256, float *cos256)
{
    if (!window256 || !cos256) return fail(FMRX_EINVAL, "audio_spectrum_tables: null argument");
    std::memcpy(window256, kTables.w, sizeof kTables.w);
    std::memcpy(cos256, kTables.c, sizeof kTables.c);
    return FMRX_OK;
}

size_t fmrx_audio_spectrum_frame(void) { return kFrame; }

size_t fmrx_audio_spectrum_bins(void) { return kBins; }

size_t fmrx_audio_spectrum_tile(void) { return kTile; }

size_t fmrx_audio_spectrum_max_bands(void) { return kMaxBands; }

int fmrx_audio_spectrum_default_edges(int *edges, int *n_bands)
{
    if (!edges || !n_bands) return fail(FMRX_EINVAL, "audio_spectrum_default_edges: null argument");
    std::memcpy(edges, audio_spectrum::kDefaultEdges, sizeof audio_spectrum::kDefaultEdges);
    *n_bands = audio_spectrum::kDefaultBands;
    return FMRX_OK;
}

int fmrx_audio_spectrum_walk(int audio_channels, const float *rows, size_t row_pitch, size_t n, const int *edges, int n_bands,
                             fmrx_audio_spectrum_state *state_in_out, fmrx_audio_spectrum_record *rec)
{
    if (!rows || !state_in_out || !rec) return fail(FMRX_EINVAL, "audio_spectrum_walk: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "audio_spectrum_walk: audio_channels must be 1 or 2");
    if (n < 1 || n > (size_t{1} << 26) || row_pitch < n) return fail(FMRX_EINVAL, "audio_spectrum_walk: %zu samples (1 .. 2^26) in rows of %zu", n, row_pitch);
    if (state_in_out->fill >= static_cast<unsigned>(kFrame)) return fail(FMRX_EINVAL, "audio_spectrum_walk: fill %u (0 .. 255)", state_in_out->fill);
    int e[kMaxBands + 1], B;
    FMRX_TRY(take_edges("audio_spectrum_walk", edges, n_bands, e, &B));
    std::memset(rec, 0, sizeof *rec);
    const unsigned fill = state_in_out->fill;
    rec->n = n;
    rec->frames = (fill + n) / kFrame;
    for (int r = 0; r < audio_channels; r++) walk_row(rows + r * row_pitch, n, e, B, fill, state_in_out->carry[r], rec->band[r]);
    state_in_out->fill = static_cast<unsigned>((fill + n) % kFrame);
    return FMRX_OK;
}

int fmrx_audio_spectrum_derive(const fmrx_audio_spectrum_record *m, int audio_channels, const int *edges, int n_bands, double audio_Fs,
                               double full_scale, fmrx_audio_spectrum_levels *out)
{
    FMRX_TRY(meter_stage::check_derive("audio_spectrum_derive", m, out, audio_channels, full_scale));
    if (!(audio_Fs > 0.0) || !std::isfinite(audio_Fs)) return fail(FMRX_EINVAL, "audio_spectrum_derive: audio_Fs %g", audio_Fs);
    int e[kMaxBands + 1], B;
    FMRX_TRY(take_edges("audio_spectrum_derive", edges, n_bands, e, &B));
    const double den = 6144.0 * (full_scale * full_scale);   // 256 sum(w^2) / 4: a full-scale sine inside a band reads 0 dBFS
    const double frames = static_cast<double>(m->frames);
    std::memset(out, 0, sizeof *out);
    for (int r = 0; r < 2; r++) {
        for (int b = 0; b < kMaxBands; b++) out->band_dbfs[r][b] = -99.0;
        out->total_dbfs[r] = -99.0;
        if (r >= audio_channels || m->frames == 0) continue;
        double total = 0.0, moment = 0.0;
        for (int b = 0; b < B; b++) {
            const double v = m->band[r][b];
            out->band_dbfs[r][b] = db(v / frames, den);
            total += v;
            moment += (e[b] + e[b + 1] - 1) / 2.0 * (audio_Fs / kFrame) * v;
        }
        out->total_dbfs[r] = db(total / frames, den);
        out->centroid_hz[r] = total > 0.0 ? moment / total : 0.0;
    }
    return FMRX_OK;
}

int fmrx_audio_spectrum_create(fmrx_audio_spectrum **out, int n_channels, int audio_channels, size_t n_audio, const int *edges, int n_bands, int device)
{
    int e[kMaxBands + 1], B;
    FMRX_TRY(take_edges("audio_spectrum_create", edges, n_bands, e, &B));
    return meter_stage::create_on_audio("audio_spectrum_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_audio_spectrum *m) -> int {
        const size_t N = n_channels;
        m->n_bands = B;
        std::memcpy(m->edges, e, sizeof e);
        FMRX_TRY(m->d_edges.alloc(B + 1));
        FMRX_HIP(hipMemcpy(m->d_edges.p, e, (B + 1) * sizeof(int), hipMemcpyHostToDevice));
        for (int k = 0; k < 2; k++) {
            FMRX_TRY(m->d_fill[k].alloc(N));
            FMRX_TRY(m->d_carry[k].alloc(m->rows() * kFrame));
            FMRX_HIP(hipMemset(m->d_fill[k].p, 0, m->d_fill[k].bytes()));
            FMRX_HIP(hipMemset(m->d_carry[k].p, 0, m->d_carry[k].bytes()));
        }
        FMRX_TRY(m->d_frames.alloc(N));
        FMRX_TRY(m->h_frames.alloc(N));
        FMRX_TRY(m->d_res.alloc(N * audio_channels * B));
        FMRX_TRY(m->h_res.alloc(m->d_res.n));
        if (n_audio > kAudioSpectrumPairMax) FMRX_TRY(m->d_tiles.alloc(audio_spectrum_tiles(n_audio) * m->rows() * B));
        return FMRX_OK;
    });
}

int fmrx_audio_spectrum_destroy(fmrx_audio_spectrum *m) { return meter_stage::destroy(m); }

int fmrx_audio_spectrum_reset(fmrx_audio_spectrum *m, int channel)
{
    return meter_stage::reset_on_audio("audio_spectrum_reset", m, channel, [&]() -> int {
        const DevBuf<unsigned> &f = m->d_fill[m->cur];
        const DevBuf<float> &c = m->d_carry[m->cur];
        const size_t per = static_cast<size_t>(m->audio_channels) * kFrame;
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

int fmrx_audio_spectrum_state_get(fmrx_audio_spectrum *m, fmrx_audio_spectrum_state *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "audio_spectrum_state_get: null argument");
    FMRX_TRY(m->wait());
    const size_t N = m->n_channels;
    const int ac = m->audio_channels;
    std::vector<unsigned> fill(N);
    std::vector<float> carry(m->rows() * kFrame);
    FMRX_HIP(hipMemcpy(fill.data(), m->d_fill[m->cur].p, N * sizeof(unsigned), hipMemcpyDeviceToHost));
    FMRX_HIP(hipMemcpy(carry.data(), m->d_carry[m->cur].p, carry.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::memset(out, 0, N * sizeof *out);
    for (size_t c = 0; c < N; c++) {
        out[c].fill = fill[c];
        for (int r = 0; r < ac; r++) std::memcpy(out[c].carry[r], carry.data() + (c * ac + r) * kFrame, fill[c] * sizeof(float));   // entries from fill on read 0
    }
    return FMRX_OK;
}

int fmrx_audio_spectrum_process_dev(fmrx_audio_spectrum *m, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    return meter_stage::read_dev("audio_spectrum_process_dev", m, launch, d_audio, row_pitch, n, stream);
}

int fmrx_audio_spectrum_collect(fmrx_audio_spectrum *m, fmrx_audio_spectrum_record *out)
{
    FMRX_TRY(meter_stage::collected("audio_spectrum_collect", m, out));
    const int N = m->n_channels, B = m->n_bands;
    std::memset(out, 0, static_cast<size_t>(N) * sizeof *out);
    for (size_t c = 0; c < static_cast<size_t>(N); c++) {
        fmrx_audio_spectrum_record &r = out[c];
        r.n = m->n;
        r.frames = m->h_frames.p[c];
        for (int k = 0; k < m->audio_channels; k++)
            for (int b = 0; b < B; b++) r.band[k][b] = field(m->h_res.p, N, k * B + b, c);
    }
    return FMRX_OK;
}

int fmrx_audio_spectrum_process(fmrx_audio_spectrum *m, const float *audio, size_t row_pitch, size_t n, fmrx_audio_spectrum_record *out)
{
    return meter_stage::read_host("audio_spectrum_process", m, launch, audio, row_pitch, n, out, [&] { return fmrx_audio_spectrum_collect(m, out); });
}

}  // extern "C"
