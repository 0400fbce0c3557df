// leveller.hip -- the loudness leveller / peak limiter stage's handle and C ABI (include/fmrx.h: fmrx_leveller_*): per channel of
// a receiver bank, a gain towards a loudness target, decided from the audio meters' K-weighted sums, and a look-ahead limiter
// below full scale, applied to the audio behind the audio meters.  Control step and gain code: leveller_control.hpp; kernels:
// kernels_leveller.hip; definition: tests/_leveller_model.py.
//
// The handle is meter_stage.hpp's stage with the control structure and the limiter's state in two buffers, one read and one
// written by a call, swapped behind it.  Its source of control data is the audio meters: the K-weighted sums and sample counts
// that an audio meters handle left on the device (from_handle), or those of the host's records (from_records).
#include "leveller_control.hpp"
#include "meter_stage.hpp"

#include <cmath>

using namespace fmrx;

struct fmrx_leveller : meter_stage::Stage<fmrx_leveller_status> {
    struct Source {   // sum_k2[0] and sum_k2[1] of every channel, and their n (or n_all for all of them where d_n_each is NULL)
        const double *d_k2a, *d_k2b;
        const unsigned long long *d_n_each;
        unsigned long long n_all;
    };
    leveller::Control control{};
    int W = 64;
    double audio_Fs = 0.0;
    DevBuf<uint32_t> d_state[2];
    int cur = 0;                              // the buffer the next call reads
    DevBuf<double> d_k2;                      // the host call only: sum_k2[0] of every channel, then sum_k2[1]
    DevBuf<unsigned long long> d_n;

    // what the audio meters' last call left on the device, if it fits the stage
    static int from_handle(const char *who, const fmrx_leveller *h, const fmrx_audio_meters *am, Source *src)
    {
        const AudioMetersSums v = audio_meters_sums(am);
        if (!v.ran) return fail(FMRX_EINVAL, "%s: the audio meters have made no call", who);
        if (v.n_channels != h->n_channels || v.ac != h->audio_channels || v.device != h->device)
            return fail(FMRX_EINVAL, "%s: the audio meters have %d channels of %d rows on device %d, the leveller %d of %d on %d", who, v.n_channels, v.ac,
                        v.device, h->n_channels, h->audio_channels, h->device);
        if (v.n != h->n_audio) return fail(FMRX_EINVAL, "%s: the audio meters' last call walked %zu samples per row, the leveller's rows have %zu", who, v.n, h->n_audio);
        const size_t N = h->n_channels;
        *src = Source{v.d_sums + 6 * N, v.d_sums + 7 * N, nullptr, v.n};   // sum_k2[0], sum_k2[1] of the field-major sums
        return FMRX_OK;
    }

    static int from_records(fmrx_leveller *h, const fmrx_audio_meter *recs, Source *src)
    {
        const size_t N = h->n_channels;
        std::vector<double> k2(2 * N);
        std::vector<unsigned long long> n(N);
        for (size_t c = 0; c < N; c++) {
            k2[c] = recs[c].sum_k2[0];
            k2[N + c] = recs[c].sum_k2[1];
            n[c] = recs[c].n;
        }
        FMRX_TRY(h->d_k2.ensure(2 * N));
        FMRX_TRY(h->d_n.ensure(N));
        FMRX_HIP(hipMemcpy(h->d_k2.p, k2.data(), k2.size() * sizeof(double), hipMemcpyHostToDevice));
        FMRX_HIP(hipMemcpy(h->d_n.p, n.data(), N * sizeof(unsigned long long), hipMemcpyHostToDevice));
        *src = Source{h->d_k2.p, h->d_k2.p + N, h->d_n.p, 0};
        return FMRX_OK;
    }
};

namespace {

int launch(fmrx_leveller *h, const meter_stage::Call<fmrx_leveller::Source> &c)
{
    FMRX_TRY(leveller_control_launch(h->control, h->audio_channels, c.src.d_k2a, c.src.d_k2b, c.src.d_n_each, c.src.n_all, h->d_status.p, h->n_channels,
                                     c.s));
    LevellerArgs a;
    a.x = c.d_in;
    a.y = c.d_out;
    a.pcm = c.d_pcm;
    a.status = h->d_status.p;
    a.state_in = h->d_state[h->cur].p;
    a.state_out = h->d_state[h->cur ^ 1].p;
    a.n_channels = h->n_channels;
    a.ac = h->audio_channels;
    a.W = h->W;
    a.wrap = c.wrap;
    a.n = h->n_audio;
    a.inv_n = h->inv_n;
    a.ceiling = h->control.ceiling;
    FMRX_TRY(leveller_apply_launch(a, c.s));
    h->cur ^= 1;
    return FMRX_OK;
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

// the leveller's own refusal, in front of the shared call
int apart(const char *who, const fmrx_leveller *h, const float *in, const float *out, const int16_t *pcm)
{
    if (!h) return fail(FMRX_EINVAL, "%s: null handle", who);
    const size_t bytes = h->rows() * h->n_audio * sizeof(float);
    if (overlap(in, bytes, out, bytes) || overlap(in, bytes, pcm, bytes / 2))
        return fail(FMRX_EINVAL, "%s: the output overlaps the input (a workgroup reads %d samples in front of the ones it writes)", who, 2 * h->W);
    return FMRX_OK;
}

template <int AC>
void walk(int W, float ceiling, float gain0, float gain1, const float *rows, size_t pitch, size_t n, uint32_t *codes, float *u, float *out,
          size_t out_pitch, uint32_t *min_code, uint32_t *limited)
{
    const size_t nc = 2 * static_cast<size_t>(W) - 2, nu = static_cast<size_t>(W) - 1;
    const int lg = leveller::log2_of(W);
    const float inv_n = static_cast<float>(1.0 / static_cast<double>(n)), gs = (gain1 - gain0) * inv_n;
    std::vector<uint32_t> q(nc + n), m(nu + n);
    std::vector<float> uu[AC];
    std::memcpy(q.data(), codes, nc * sizeof(uint32_t));
    for (int r = 0; r < AC; r++) {
        uu[r].resize(nu + n);
        std::memcpy(uu[r].data(), u + r * nu, nu * sizeof(float));
    }
    for (size_t k = 0; k < n; k++) {
        const float g = std::fmaf(static_cast<float>(k + 1), gs, gain0);
        uint32_t c = leveller::kOne;
        for (int r = 0; r < AC; r++) {
            const float v = rows[r * pitch + k] * g;
            uu[r][nu + k] = v;
            const uint32_t cr = leveller::code_of(std::fabs(v), ceiling);
            c = cr < c ? cr : c;
        }
        q[nc + k] = c;
    }
    for (size_t j = 0; j < nu + n; j++) {   // m of sample j - (W - 1): the window ends at q's index j + W - 1
        uint32_t v = q[j];
        for (int i = 1; i < W; i++) v = q[j + i] < v ? q[j + i] : v;
        m[j] = v;
    }
    uint32_t mn = leveller::kOne, cnt = 0;
    for (size_t k = 0; k < n; k++) {
        uint32_t sum = 0;
        for (int i = 0; i < W; i++) sum += m[k + i];
        const uint32_t s = sum >> lg;
        const float sf = static_cast<float>(s) * 0x1p-24f;
        for (int r = 0; r < AC; r++) out[r * out_pitch + k] = uu[r][k] * sf;
        mn = s < mn ? s : mn;
        cnt += s < leveller::kOne ? 1u : 0u;
    }
    std::memcpy(codes, q.data() + n, nc * sizeof(uint32_t));
    for (int r = 0; r < AC; r++) std::memcpy(u + r * nu, uu[r].data() + n, nu * sizeof(float));
    if (min_code) *min_code = mn;
    if (limited) *limited = cnt;
}

}  // namespace

extern "C" {

int fmrx_leveller_defaults(fmrx_leveller_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "leveller_defaults: null argument");
    *p = fmrx_leveller_params{-23.0, 12.0, 20.0, -50.0, 0.2, 0.02, -1.0, 2.0};
    return FMRX_OK;
}

int fmrx_leveller_control(const fmrx_leveller_params *p, int audio_channels, const fmrx_audio_meter *rec, fmrx_leveller_status *state_in_out)
{
    if (!p || !rec || !state_in_out) return fail(FMRX_EINVAL, "leveller_control: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "leveller_control: audio_channels must be 1 or 2");
    leveller::Control c;
    if (!leveller::control_make(*p, &c)) return fail(FMRX_EINVAL, "leveller_control: parameters (fmrx.h lists the conditions)");
    leveller::control_step(c, audio_channels, rec->n, rec->sum_k2[0], rec->sum_k2[1], *state_in_out);
    return FMRX_OK;
}

int fmrx_leveller_ceiling(const fmrx_leveller_params *p, float *ceiling)
{
    if (!p || !ceiling) return fail(FMRX_EINVAL, "leveller_ceiling: null argument");
    leveller::Control c;
    if (!leveller::control_make(*p, &c)) return fail(FMRX_EINVAL, "leveller_ceiling: parameters (fmrx.h lists the conditions)");
    *ceiling = c.ceiling;
    return FMRX_OK;
}

int fmrx_leveller_derive(const fmrx_leveller_status *st, fmrx_leveller_levels *out)
{
    if (!st || !out) return fail(FMRX_EINVAL, "leveller_derive: null argument");
    const auto clamp = [](double v) { return v < -99.0 ? -99.0 : (v > 99.0 ? 99.0 : v); };
    out->loudness_lkfs = db(st->loud_ms, 1.0, -leveller::kLkfsOffset);
    out->gain_db = st->gain > 0.0 ? clamp(20.0 * std::log10(st->gain)) : -99.0;
    out->reduction_db = st->min_code > 0 ? clamp(20.0 * std::log10(static_cast<double>(st->min_code) / 16777216.0)) : -99.0;
    return FMRX_OK;
}

size_t fmrx_leveller_tile(int lookahead) { return leveller::good_lookahead(lookahead) ? static_cast<size_t>(leveller::kSpan - 2 * lookahead) : 0; }

int fmrx_leveller_walk(int audio_channels, int lookahead, float ceiling, float gain0, float gain1, const float *rows, size_t row_pitch, size_t n,
                       uint32_t *codes, float *u, float *out, size_t out_pitch, uint32_t *min_code, uint32_t *limited)
{
    if (!rows || !codes || !u || !out) return fail(FMRX_EINVAL, "leveller_walk: null argument");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "leveller_walk: audio_channels must be 1 or 2");
    if (!leveller::good_lookahead(lookahead)) return fail(FMRX_EINVAL, "leveller_walk: lookahead %d: a power of two in 8 .. 128", lookahead);
    if (!(ceiling >= 1.17549435e-38f) || !(ceiling - ceiling == 0.0f)) return fail(FMRX_EINVAL, "leveller_walk: ceiling %g", ceiling);
    if (n < 1 || n > (size_t{1} << 26) || row_pitch < n || out_pitch < n)
        return fail(FMRX_EINVAL, "leveller_walk: %zu samples (1 .. 2^26) in rows of %zu and %zu", n, row_pitch, out_pitch);
    if (audio_channels == 2) walk<2>(lookahead, ceiling, gain0, gain1, rows, row_pitch, n, codes, u, out, out_pitch, min_code, limited);
    else walk<1>(lookahead, ceiling, gain0, gain1, rows, row_pitch, n, codes, u, out, out_pitch, min_code, limited);
    return FMRX_OK;
}

int fmrx_leveller_create(fmrx_leveller **out, const fmrx_leveller_params *p, double audio_Fs, int n_channels, int audio_channels, size_t n_audio,
                         int lookahead, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "leveller_create: null argument");
    leveller::Control c;
    if (!leveller::control_make(*p, &c)) return fail(FMRX_EINVAL, "leveller_create: parameters (fmrx.h lists the conditions)");
    if (!std::isfinite(audio_Fs) || audio_Fs < 8000.0 || audio_Fs > 768000.0) return fail(FMRX_EINVAL, "leveller_create: audio_Fs %g (finite, 8000 .. 768000)", audio_Fs);
    const int W = lookahead == 0 ? 64 : lookahead;
    if (!leveller::good_lookahead(W)) return fail(FMRX_EINVAL, "leveller_create: lookahead %d: a power of two in 8 .. 128, or 0 for 64", lookahead);
    return meter_stage::create("leveller_create", out, n_channels, audio_channels, n_audio, device, [&](fmrx_leveller *h) -> int {
        h->control = c;
        h->W = W;
        h->audio_Fs = audio_Fs;
        for (auto &b : h->d_state) {
            FMRX_TRY(b.alloc(static_cast<size_t>(n_channels) * leveller_state_words(audio_channels, W)));
            FMRX_HIP(hipMemset(b.p, 0, b.bytes()));
        }
        return FMRX_OK;
    });
}

int fmrx_leveller_destroy(fmrx_leveller *h) { return meter_stage::destroy(h); }

int fmrx_leveller_reset(fmrx_leveller *h, int channel)
{
    return meter_stage::reset("leveller_reset", h, channel, [&]() -> int {   // the limiter's state with the status row: zeros are fresh
        DevBuf<uint32_t> &b = h->d_state[h->cur];
        const size_t words = leveller_state_words(h->audio_channels, h->W);
        if (channel < 0) FMRX_HIP(hipMemset(b.p, 0, b.bytes()));
        else FMRX_HIP(hipMemset(b.p + static_cast<size_t>(channel) * words, 0, words * sizeof(uint32_t)));
        return FMRX_OK;
    });
}

size_t fmrx_leveller_latency(const fmrx_leveller *h) { return h ? static_cast<size_t>(h->W - 1) : 0; }

int fmrx_leveller_process_dev(fmrx_leveller *h, const fmrx_audio_meters *am, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy,
                              void *stream)
{
    FMRX_TRY(apart("leveller_process_dev", h, d_in, d_out, d_pcm16));
    return meter_stage::process_dev("leveller_process_dev", h, launch, am, d_in, d_out, d_pcm16, pcm_policy, stream);
}

int fmrx_leveller_process(fmrx_leveller *h, const fmrx_audio_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    FMRX_TRY(apart("leveller_process", h, in, out, pcm16));
    return meter_stage::process("leveller_process", h, launch, recs, in, out, pcm16, pcm_policy);
}

int fmrx_leveller_status_get(fmrx_leveller *h, fmrx_leveller_status *out) { return meter_stage::status_get("leveller_status_get", h, out); }

}  // extern "C"
