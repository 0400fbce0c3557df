// tuner.hip -- the wideband tuner's handle and C ABI (include/fmrx.h: fmrx_tuner_*): one wide I/Q capture (u8, s8 or
// little-endian s16) at Fs_w in, N channels' u8 I/Q streams at rf_Fs = Fs_w * U / D out, written straight into a receiver
// bank's input slots (fmrx_channels_input_layout).  One host path for every rate: fmrx_tuner_create and _create_ex make the
// handle of U = 1, D = R (the integer tuner), fmrx_tuner_create_rational that of any U / D (section
// 4.9.2), and U = 1 there is the same handle.  The taps are U phases of Tp = ceil(T / U) taps, and a call takes a multiple of
// D wide samples.  Arithmetic: tuner_host.hpp, defined by tests/_tuner_model.py, tests/_tuner_formats_model.py (the input
// formats) and tests/_tuner_rational_model.py (U > 1).  Kernels: tuner_launch (kernels_tuner.hip) picks them: the integer
// matrix kernels for U = 1, D <= 32, those of kernels_tuner_rational.hip for the other rates, the generic kernel for both.
//
// State carried by the handle: the last `front` raw values of the stream (front = 2 (Tp - 1) rounded up to 16; zero samples
// at the start: bytes 0x80 for u8, 0x00 for the signed formats) in one of two device buffers that swap roles every call,
// and the wide-sample counter (uint64, used mod 2^32).
// Channel parameters live on the host (taps as int16 pairs, frequency word, scale exponent, the matrix kernel's operand
// image); fmrx_tuner_set_channel changes the host copy and marks the channel, the next call uploads what changed.
#include "fmrx_internal.hpp"
#include "tuner_host.hpp"

#include <algorithm>

using namespace fmrx;

struct fmrx_tuner {
    int device = 0, T = 0, n_channels = 0, format = kTunerU8;
    int U = 1, D = 0;                    // the rate: (1, R) for the integer tuner
    TunerShape sh;
    long max_wide = 0;
    bool mfma = true;
    size_t group_bytes = 0;
    std::vector<float> h;
    std::vector<int16_t> re, im;         // [n_channels][U * Tp], phase-major
    std::vector<uint2> chan;             // {w, s + 15 + B}
    std::vector<int2> kconst;            // 16-bit matrix kernel: [n_channels][U], per phase 128 * {sum(re - im), sum(im + re)}
    std::vector<int8_t> img;             // matrix kernel: [groups][group_bytes]
    std::vector<uint8_t> dirty;
    size_t n_dirty = 0;
    DevBuf<int8_t> d_img;
    DevBuf<int16_t> d_re, d_im;
    DevBuf<uint2> d_chan;
    DevBuf<int2> d_kconst;
    DevBuf<unsigned> d_table;
    DevBuf<uint8_t> d_hist[2];
    int cur = 0;
    DevBuf<unsigned long long> d_levels;
    DevBuf<uint8_t> d_wide, d_out;       // fmrx_tuner_process only
    size_t out_pitch = 0;
    uint64_t counter = 0;
    hipStream_t last_stream = nullptr;
    bool ran = false;
    bool wide_planes() const { return mfma && format == kTunerS16; }
    size_t n_taps() const { return static_cast<size_t>(U) * sh.Tp; }   // int16 pairs per channel
};

static_assert(FMRX_TUNER_U8 == kTunerU8 && FMRX_TUNER_S8 == kTunerS8 && FMRX_TUNER_S16 == kTunerS16, "fmrx.h and tuner_host.hpp");

namespace {

int n_groups(const fmrx_tuner *t) { return (t->n_channels + kTunerGroup - 1) / kTunerGroup; }

// one channel's integers into the host copies
int design_channel(fmrx_tuner *t, int c, double f_c, double Fs_w, double gain)
{
    uint32_t w = 0;
    int s = 0;
    const size_t nt = t->n_taps();
    const int U = t->U, Tp = t->sh.Tp;
    std::vector<int16_t> re(nt), im(nt);
    if (const char *why = tuner_design(t->h.data(), t->T, U, Fs_w, f_c, gain, &w, &s, re.data(), im.data()))
        return fail(FMRX_EINVAL, "tuner channel %d: %s", c, why);
    if (s > tuner_max_shift(t->format))
        return fail(FMRX_EINVAL, "tuner channel %d: gain x taps too small for 16-bit input (scale exponent %d outside -14 .. %d)", c, s,
                    tuner_max_shift(t->format));
    std::copy(re.begin(), re.end(), t->re.begin() + c * nt);
    std::copy(im.begin(), im.end(), t->im.begin() + c * nt);
    t->chan[c] = make_uint2(w, static_cast<unsigned>(s + 15 + tuner_extra_bits(t->format)));
    if (t->wide_planes())
        for (int p = 0; p < U; p++) {
            long long sr = 0, si = 0;
            for (int j = 0; j < Tp; j++) {
                sr += re[p * Tp + j] - im[p * Tp + j];
                si += im[p * Tp + j] + re[p * Tp + j];
            }
            t->kconst[static_cast<size_t>(c) * U + p] = make_int2(static_cast<int>(128 * sr), static_cast<int>(128 * si));   // a phase's sum < 2^31
        }
    if (t->mfma) tuner_fill_image(t->img.data() + static_cast<size_t>(c / kTunerGroup) * t->group_bytes, t->sh, c % kTunerGroup, re.data(), im.data());
    if (!t->dirty[c]) {
        t->dirty[c] = 1;
        t->n_dirty++;
    }
    return FMRX_OK;
}

// what set_channel changed since the last call -> device (ordered on `stream`, complete when this returns)
int upload_dirty(fmrx_tuner *t, hipStream_t stream)
{
    if (!t->n_dirty) return FMRX_OK;
    const size_t N = t->n_channels, T = t->n_taps(), K = t->U;
    if (t->n_dirty == N) {
        FMRX_HIP(hipMemcpyAsync(t->d_chan.p, t->chan.data(), N * sizeof(uint2), hipMemcpyHostToDevice, stream));
        if (t->wide_planes()) FMRX_HIP(hipMemcpyAsync(t->d_kconst.p, t->kconst.data(), N * K * sizeof(int2), hipMemcpyHostToDevice, stream));
        if (t->mfma) {
            FMRX_HIP(hipMemcpyAsync(t->d_img.p, t->img.data(), t->img.size(), hipMemcpyHostToDevice, stream));
        } else {
            FMRX_HIP(hipMemcpyAsync(t->d_re.p, t->re.data(), N * T * sizeof(int16_t), hipMemcpyHostToDevice, stream));
            FMRX_HIP(hipMemcpyAsync(t->d_im.p, t->im.data(), N * T * sizeof(int16_t), hipMemcpyHostToDevice, stream));
        }
    } else {
        for (size_t c = 0; c < N; c++) {
            if (!t->dirty[c]) continue;
            FMRX_HIP(hipMemcpyAsync(t->d_chan.p + c, t->chan.data() + c, sizeof(uint2), hipMemcpyHostToDevice, stream));
            if (t->wide_planes())
                FMRX_HIP(hipMemcpyAsync(t->d_kconst.p + c * K, t->kconst.data() + c * K, K * sizeof(int2), hipMemcpyHostToDevice, stream));
            if (t->mfma) {
                const size_t off = c / kTunerGroup * t->group_bytes;
                FMRX_HIP(hipMemcpyAsync(t->d_img.p + off, t->img.data() + off, t->group_bytes, hipMemcpyHostToDevice, stream));
            } else {
                FMRX_HIP(hipMemcpyAsync(t->d_re.p + c * T, t->re.data() + c * T, T * sizeof(int16_t), hipMemcpyHostToDevice, stream));
                FMRX_HIP(hipMemcpyAsync(t->d_im.p + c * T, t->im.data() + c * T, T * sizeof(int16_t), hipMemcpyHostToDevice, stream));
            }
        }
    }
    FMRX_HIP(hipStreamSynchronize(stream));   // the host copies are pageable and may change again right after the call
    std::fill(t->dirty.begin(), t->dirty.end(), 0);
    t->n_dirty = 0;
    return FMRX_OK;
}

int clear_state(fmrx_tuner *t)
{
    if (t->ran) FMRX_HIP(hipStreamSynchronize(t->last_stream));
    FMRX_HIP(hipMemset(t->d_hist[0].p, tuner_zero_byte(t->format), t->d_hist[0].bytes()));
    FMRX_HIP(hipMemset(t->d_hist[1].p, tuner_zero_byte(t->format), t->d_hist[1].bytes()));
    FMRX_HIP(hipMemset(t->d_levels.p, 0, t->d_levels.bytes()));
    t->cur = 0;
    t->counter = 0;
    return FMRX_OK;
}

// The handle of the rate U / D, already checked by the caller; fn: the public function's name, for the messages.
int create(fmrx_tuner **out, const char *fn, int U, int D, const float *h, int taps, int n_channels, size_t max_wide_samples, int format,
           int device)
{
    if (!out || !h) return fail(FMRX_EINVAL, "%s: null argument", fn);
    if (!tuner_format_ok(format)) return fail(FMRX_EINVAL, "%s: format %d (FMRX_TUNER_U8, _S8 or _S16)", fn, format);
    if (taps < 2 || taps > kTunerMaxTaps) return fail(FMRX_EINVAL, "%s: %d taps (2 .. %d)", fn, taps, kTunerMaxTaps);
    if (n_channels < 1 || n_channels > 65536) return fail(FMRX_EINVAL, "%s: n_channels must be 1 .. 65536", fn);
    if (max_wide_samples < static_cast<size_t>(D) || max_wide_samples % D || max_wide_samples / D * U > (1u << 24))
        return fail(FMRX_EINVAL, "%s: max_wide_samples %zu must be a multiple of D = %d (the decimation), at most 2^24 outputs per call", fn,
                    max_wide_samples, D);
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    fmrx_tuner *t = new fmrx_tuner;
    t->device = device;
    t->U = U;
    t->D = D;
    t->T = taps;
    t->n_channels = n_channels;
    t->format = format;
    t->max_wide = static_cast<long>(max_wide_samples);
    t->sh = tuner_shape(taps, U, D);
    // The matrix kernels' range (tuner_plan_info); outside it, and under tuner_variant = 1, the generic kernel runs.  The integer
    // tuner (D <= 32, its plan fixed) is always inside: its largest window, D = 32, T = 250 .. 256, S16, takes 52,320 bytes of LDS.
    t->mfma = tuner_plan_info(U, D, taps, format, n_channels, 0, options_snapshot().tuner_variant == 0).matrix;
    t->group_bytes = tuner_group_image_bytes(t->sh);
    t->h.assign(h, h + taps);
    auto body = [&]() -> int {
        const size_t N = n_channels, T = t->n_taps(), K = U;
        t->re.assign(N * T, 0);
        t->im.assign(N * T, 0);
        t->chan.assign(N, make_uint2(0, 1));
        if (t->wide_planes()) t->kconst.assign(N * K, make_int2(0, 0));
        t->dirty.assign(N, 0);
        if (t->mfma) t->img.assign(static_cast<size_t>(n_groups(t)) * t->group_bytes, 0);
        // every channel starts at the capture's centre with gain 1; designed once, copied to the rest
        FMRX_TRY(design_channel(t, 0, 0.0, 1.0, 1.0));
        for (size_t c = 1; c < N; c++) {
            std::copy(t->re.begin(), t->re.begin() + T, t->re.begin() + c * T);
            std::copy(t->im.begin(), t->im.begin() + T, t->im.begin() + c * T);
            t->chan[c] = t->chan[0];
            if (t->wide_planes()) std::copy(t->kconst.begin(), t->kconst.begin() + K, t->kconst.begin() + c * K);
            if (t->mfma && c < static_cast<size_t>(kTunerGroup)) tuner_fill_image(t->img.data(), t->sh, static_cast<int>(c), t->re.data(), t->im.data());
        }
        if (t->mfma)
            for (int g = 1; g < n_groups(t); g++)
                std::copy(t->img.begin(), t->img.begin() + t->group_bytes, t->img.begin() + static_cast<size_t>(g) * t->group_bytes);
        std::fill(t->dirty.begin(), t->dirty.end(), 1);
        t->n_dirty = N;
        FMRX_TRY(t->d_chan.alloc(N));
        if (t->wide_planes()) FMRX_TRY(t->d_kconst.alloc(N * K));
        if (t->mfma) {
            FMRX_TRY(t->d_img.alloc(t->img.size()));
        } else {
            FMRX_TRY(t->d_re.alloc(N * T));
            FMRX_TRY(t->d_im.alloc(N * T));
        }
        std::vector<int16_t> c(kTunerTableSize), s(kTunerTableSize);
        std::vector<unsigned> tab(kTunerTableSize);
        tuner_table(c.data(), s.data());
        for (int i = 0; i < kTunerTableSize; i++)
            tab[i] = static_cast<unsigned>(static_cast<uint16_t>(c[i])) | (static_cast<unsigned>(static_cast<uint16_t>(s[i])) << 16);
        FMRX_TRY(t->d_table.alloc(kTunerTableSize));
        FMRX_HIP(hipMemcpy(t->d_table.p, tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        FMRX_TRY(t->d_hist[0].alloc(static_cast<size_t>(t->sh.front) * tuner_value_bytes(format)));
        FMRX_TRY(t->d_hist[1].alloc(static_cast<size_t>(t->sh.front) * tuner_value_bytes(format)));
        FMRX_TRY(t->d_levels.alloc(2 * N));
        return clear_state(t);
    };
    const int rc = body();
    if (rc != FMRX_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_tuner_design(const float *h, int taps, double Fs_w, double f_c, double gain, uint32_t *w, int *s, int16_t *re, int16_t *im)
{
    if (!h || !w || !s || !re || !im) return fail(FMRX_EINVAL, "tuner_design: null argument");
    if (const char *why = tuner_design(h, taps, 1, Fs_w, f_c, gain, w, s, re, im)) return fail(FMRX_EINVAL, "tuner_design: %s", why);
    return FMRX_OK;
}

int fmrx_tuner_table(int16_t *cos_q15, int16_t *sin_q15, size_t *n)
{
    if (!n) return fail(FMRX_EINVAL, "tuner_table: null argument");
    *n = kTunerTableSize;
    if (cos_q15 && sin_q15) tuner_table(cos_q15, sin_q15);
    return FMRX_OK;
}

int fmrx_tuner_create(fmrx_tuner **out, int R, const float *h, int taps, int n_channels, size_t max_wide_samples, int device)
{
    return fmrx_tuner_create_ex(out, R, h, taps, n_channels, max_wide_samples, FMRX_TUNER_U8, device);
}

int fmrx_tuner_create_ex(fmrx_tuner **out, int R, const float *h, int taps, int n_channels, size_t max_wide_samples, int format, int device)
{
    if (R < 2 || R > kTunerMaxR) return fail(FMRX_EINVAL, "tuner_create: decimation %d (2 .. %d)", R, kTunerMaxR);
    return create(out, "tuner_create", 1, R, h, taps, n_channels, max_wide_samples, format, device);
}

int fmrx_tuner_design_rational(const float *h, int taps, int U, double Fs_w, double f_c, double gain, uint32_t *w, int *s, int16_t *re,
                               int16_t *im)
{
    if (!h || !w || !s || !re || !im) return fail(FMRX_EINVAL, "tuner_design_rational: null argument");
    if (const char *why = tuner_design(h, taps, U, Fs_w, f_c, gain, w, s, re, im)) return fail(FMRX_EINVAL, "tuner_design_rational: %s", why);
    return FMRX_OK;
}

int fmrx_tuner_create_rational(fmrx_tuner **out, int U, int D, const float *h, int taps, int n_channels, size_t max_wide_samples, int format,
                               int device)
{
    if (const char *why = tuner_ratio_check(U, D)) return fail(FMRX_EINVAL, "tuner_create_rational: ratio %d/%d: %s", U, D, why);
    return create(out, "tuner_create_rational", U, D, h, taps, n_channels, max_wide_samples, format, device);
}

int fmrx_tuner_ratio(const fmrx_tuner *t, int *U, int *D)
{
    if (!t || !U || !D) return fail(FMRX_EINVAL, "tuner_ratio: null argument");
    *U = t->U;
    *D = t->D;
    return FMRX_OK;
}

int fmrx_tuner_destroy(fmrx_tuner *t)
{
    if (!t) return FMRX_OK;
    (void)hipSetDevice(t->device);
    if (t->ran) (void)hipStreamSynchronize(t->last_stream);
    delete t;
    return FMRX_OK;
}

int fmrx_tuner_reset(fmrx_tuner *t)
{
    if (!t) return fail(FMRX_EINVAL, "tuner_reset: null handle");
    FMRX_HIP(hipSetDevice(t->device));
    return clear_state(t);
}

int fmrx_tuner_set_channel(fmrx_tuner *t, int channel, double f_c_hz, double Fs_w, double gain)
{
    if (!t) return fail(FMRX_EINVAL, "tuner_set_channel: null handle");
    if (channel < 0 || channel >= t->n_channels) return fail(FMRX_EINVAL, "tuner_set_channel: channel %d of %d", channel, t->n_channels);
    return design_channel(t, channel, f_c_hz, Fs_w, gain);
}

int fmrx_tuner_plan(const fmrx_tuner *t, size_t n_wide, fmrx_tuner_plan_info *out)
{
    if (!t || !out) return fail(FMRX_EINVAL, "tuner_plan: null argument");
    if (n_wide == 0 || n_wide % t->D || n_wide > static_cast<size_t>(t->max_wide))
        return fail(FMRX_EINVAL, "tuner_plan: n_wide = %zu wide samples: a non-zero multiple of the decimation %d, at most %ld", n_wide, t->D,
                    t->max_wide);
    const TunerPlanInfo p = tuner_plan_info(t->U, t->D, t->T, t->format, t->n_channels, static_cast<long>(n_wide), t->mfma);
    out->matrix = p.matrix;
    out->tiles = p.tiles;
    out->via_lds = p.via_lds;
    out->lds_bytes = p.lds_bytes;
    out->n_steps = p.n_steps;
    out->steps_per_wg = p.steps_per_wg;
    out->grid_x = p.grid_x;
    out->grid_y = p.grid_y;
    return FMRX_OK;
}

int fmrx_tuner_format(const fmrx_tuner *t) { return t ? t->format : -1; }

size_t fmrx_tuner_sample_bytes(const fmrx_tuner *t) { return t ? 2 * static_cast<size_t>(tuner_value_bytes(t->format)) : 0; }

size_t fmrx_tuner_n_out_bytes(const fmrx_tuner *t, size_t n_wide) { return t && n_wide % t->D == 0 ? 2 * (n_wide / t->D) * t->U : 0; }

int fmrx_tuner_process_dev(fmrx_tuner *t, const uint8_t *d_wide, size_t n_wide, uint8_t *d_out_first, size_t pitch_bytes, void *stream)
{
    if (!t || !d_wide || !d_out_first) return fail(FMRX_EINVAL, "tuner_process_dev: null argument");
    if (n_wide == 0 || n_wide % t->D || n_wide > static_cast<size_t>(t->max_wide))
        return fail(FMRX_EINVAL, "tuner_process_dev: n_wide = %zu wide samples: a non-zero multiple of the decimation %d, at most %ld", n_wide,
                    t->D, t->max_wide);
    if (reinterpret_cast<uintptr_t>(d_wide) % 16) return fail(FMRX_EINVAL, "tuner_process_dev: d_wide must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out_first) % 16 || pitch_bytes % 16)
        return fail(FMRX_EINVAL, "tuner_process_dev: d_out_first and pitch_bytes must be multiples of 16 bytes");
    if (t->n_channels > 1 && pitch_bytes < fmrx_tuner_n_out_bytes(t, n_wide))
        return fail(FMRX_EINVAL, "tuner_process_dev: pitch of %zu bytes is shorter than a channel's %zu output bytes", pitch_bytes,
                    fmrx_tuner_n_out_bytes(t, n_wide));
    FMRX_HIP(hipSetDevice(t->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    FMRX_TRY(upload_dirty(t, s));
    FMRX_HIP(hipMemsetAsync(t->d_levels.p, 0, t->d_levels.bytes(), s));
    TunerLaunch a;
    a.mfma = t->mfma;
    a.format = t->format;
    a.kconst = t->d_kconst.p;
    a.x = d_wide;
    a.n_bytes = static_cast<long>(2 * n_wide);
    a.hist = t->d_hist[t->cur].p;
    a.hist_next = t->d_hist[t->cur ^ 1].p;
    a.a_img = t->d_img.p;
    a.taps_re = t->d_re.p;
    a.taps_im = t->d_im.p;
    a.chan = t->d_chan.p;
    a.table = t->d_table.p;
    a.out = d_out_first;
    a.pitch = static_cast<long>(pitch_bytes);
    a.n_channels = t->n_channels;
    a.U = t->U;
    a.D = t->D;
    a.Tp = t->sh.Tp;
    a.front = t->sh.front;
    a.ks = t->sh.ks;
    a.ksp = t->sh.ksp;
    a.n0 = static_cast<unsigned>(t->counter & 0xffffffffu);
    a.levels = t->d_levels.p;
    FMRX_TRY(tuner_launch(a, s));
    t->cur ^= 1;
    t->counter += n_wide;
    t->last_stream = s;
    t->ran = true;
    return FMRX_OK;
}

int fmrx_tuner_process(fmrx_tuner *t, const uint8_t *wide, size_t n_wide, uint8_t *out)
{
    if (!t || !wide || !out) return fail(FMRX_EINVAL, "tuner_process: null argument");
    FMRX_HIP(hipSetDevice(t->device));
    if (!t->d_wide.p) {
        t->out_pitch = (fmrx_tuner_n_out_bytes(t, static_cast<size_t>(t->max_wide)) + 15) / 16 * 16;
        FMRX_TRY(t->d_wide.alloc(fmrx_tuner_sample_bytes(t) * static_cast<size_t>(t->max_wide)));
        FMRX_TRY(t->d_out.alloc(t->out_pitch * t->n_channels));
    }
    if (n_wide == 0 || n_wide % t->D || n_wide > static_cast<size_t>(t->max_wide))
        return fail(FMRX_EINVAL, "tuner_process: n_wide = %zu wide samples: a non-zero multiple of the decimation %d, at most %ld", n_wide, t->D,
                    t->max_wide);
    FMRX_HIP(hipMemcpy(t->d_wide.p, wide, fmrx_tuner_sample_bytes(t) * n_wide, hipMemcpyHostToDevice));
    FMRX_TRY(fmrx_tuner_process_dev(t, t->d_wide.p, n_wide, t->d_out.p, t->out_pitch, nullptr));
    FMRX_HIP(hipStreamSynchronize(nullptr));
    const size_t row = fmrx_tuner_n_out_bytes(t, n_wide);
    FMRX_HIP(hipMemcpy2D(out, row, t->d_out.p, t->out_pitch, row, t->n_channels, hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_tuner_levels(fmrx_tuner *t, uint64_t *clipped, uint64_t *power)
{
    if (!t || !clipped || !power) return fail(FMRX_EINVAL, "tuner_levels: null argument");
    FMRX_HIP(hipSetDevice(t->device));
    if (t->ran) FMRX_HIP(hipStreamSynchronize(t->last_stream));
    std::vector<unsigned long long> lv(2 * static_cast<size_t>(t->n_channels));
    FMRX_HIP(hipMemcpy(lv.data(), t->d_levels.p, lv.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int c = 0; c < t->n_channels; c++) {
        clipped[c] = lv[2 * c];
        power[c] = lv[2 * c + 1];
    }
    return FMRX_OK;
}

}  // extern "C"
