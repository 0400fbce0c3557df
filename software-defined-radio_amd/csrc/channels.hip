// channels.hip -- a bank of N independent receivers per device call: the C ABI (include/fmrx.h: fmrx_channels_*) over one Bank.
//
// The reference runs one pipeline per process (src/project.cpp:460-468: one PARAMS / STATES set); a receiver bank is N
// processes.  A live channel delivers reference-size blocks (51 200 complex samples every 21.3 ms at 2.4 MS/s): far too little
// work for one launch to fill the chip, and N launches per block period cost N times the launch latency.  A bank processes the
// current block of N channels in a few launches; every kind of bank is bank.hip's.  The handle adds what a caller of the C ABI
// needs around it: the device, a stream and device-side outputs for the host-array call, the copy of a call's input into the
// slots, and the optional de-emphasis behind the bank.
#include "bank_kernels.hpp"

using namespace fmrx;

struct fmrx_channels {
    fmrx_params p{};
    int n_channels = 0, device = 0, audio_channels = 1;
    size_t block_bytes = 0;      // bytes per channel and call
    size_t n_audio = 0;          // audio samples per channel and call (the bank's)
    Options opt;
    hipStream_t stream = nullptr;
    DevBuf<int16_t> pcm_out;
    DevBuf<float> f32_out;
    // de-emphasis (kernels_deemph.hip; off by default): while it is on, the bank writes f32 [n_channels][audio_channels][n_audio]
    // into de.in and no PCM; one pass over its n_channels * audio_channels rows, behind the bank's call, writes the caller's arrays
    Deemph de;
    std::unique_ptr<Bank> bank;
};

namespace {

// channel-major array [n_channels][block_bytes] -> the block region of every slot: one strided copy
int load_slots(fmrx_channels *c, const uint8_t *iq, hipMemcpyKind kind, hipStream_t s)
{
    uint8_t *first;
    size_t pitch;
    bank_input_layout(c->bank.get(), &first, &pitch);
    FMRX_HIP(hipMemcpy2DAsync(first, pitch, iq, c->block_bytes, c->block_bytes, c->n_channels, kind, s));
    return FMRX_OK;
}

// the bank, then the stream and the device-side outputs of the host-array entry point
int create_body(fmrx_channels *c, int exact)
{
    FMRX_TRY(bank_create(c->bank, c->p, c->n_channels, c->audio_channels, exact, c->block_bytes, c->opt));
    c->n_audio = bank_n_audio(c->bank.get());
    FMRX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    FMRX_TRY(c->pcm_out.alloc(c->n_audio * c->n_channels * c->audio_channels));
    FMRX_TRY(c->f32_out.alloc(c->n_audio * c->n_channels * c->audio_channels));
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_channels_create(fmrx_channels **out, const fmrx_params *p, int n_channels, size_t block_bytes, int device)
{
    return fmrx_channels_create_ex(out, p, n_channels, 1, 0, block_bytes, device);
}

int fmrx_channels_create_ex(fmrx_channels **out, const fmrx_params *p, int n_channels, int audio_channels, int exact,
                            size_t block_bytes, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "channels_create: null argument");
    if (n_channels < 1) return fail(FMRX_EINVAL, "channels_create: n_channels must be >= 1");
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "channels_create: audio_channels must be 1 (mono) or 2 (stereo)");
    // integer-decimation modes: whole audio samples; resampling modes: the finer rule (n_if * U % D == 0) is checked by the bank,
    // as is the block's length against the history a channel carries
    const size_t unit = static_cast<size_t>(2) * p->rf_decim * (p->audio_upsamp ? 1 : p->audio_decim);
    if (block_bytes == 0 || block_bytes % unit || block_bytes % 16)
        return fail(FMRX_EINVAL, "channels_create: block_bytes must be a multiple of 16 and of %zu", unit);
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    fmrx_channels *c = new fmrx_channels;
    c->p = *p;
    c->n_channels = n_channels;
    c->device = device;
    c->block_bytes = block_bytes;
    c->audio_channels = audio_channels;
    c->opt = options_snapshot();
    const int rc = create_body(c, exact);
    if (rc != FMRX_OK) {
        fmrx_channels_destroy(c);
        return rc;
    }
    *out = c;
    return FMRX_OK;
}

// A call through fmrx_channels_process_dev runs on the caller's stream, and a stereo bank's on its internal streams too: the device
// is waited for, not the handle's stream alone, before anything a queued kernel may still read or write is freed.
int fmrx_channels_destroy(fmrx_channels *c)
{
    if (!c) return FMRX_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    (void)hipDeviceSynchronize();
    delete c;
    return FMRX_OK;
}

size_t fmrx_channels_n_audio(const fmrx_channels *c) { return c ? c->n_audio : 0; }

int fmrx_channels_input_layout(const fmrx_channels *c, uint8_t **d_first_block, size_t *pitch_bytes)
{
    if (!c || !d_first_block || !pitch_bytes) return fail(FMRX_EINVAL, "channels_input_layout: null argument");
    bank_input_layout(c->bank.get(), d_first_block, pitch_bytes);
    return FMRX_OK;
}

int fmrx_channels_demod_layout(const fmrx_channels *c, const float **d_row0, size_t *pitch, size_t *n_if)
{
    if (!c || !d_row0 || !pitch || !n_if) return fail(FMRX_EINVAL, "channels_demod_layout: null argument");
    return bank_demod_layout(c->bank.get(), d_row0, pitch, n_if);
}

int fmrx_channels_reset(fmrx_channels *c, int channel)
{
    if (!c) return fail(FMRX_EINVAL, "channels_reset: null handle");
    if (channel >= c->n_channels) return fail(FMRX_EINVAL, "channels_reset: channel %d of %d", channel, c->n_channels);
    FMRX_HIP(hipSetDevice(c->device));
    FMRX_HIP(hipDeviceSynchronize());
    FMRX_TRY(c->de.reset(channel < 0 ? 0 : static_cast<long>(channel) * c->audio_channels,
                         static_cast<long>(channel < 0 ? c->n_channels : 1) * c->audio_channels, nullptr));
    FMRX_HIP(hipDeviceSynchronize());
    return bank_reset(c->bank.get(), channel);
}

int fmrx_channels_process_dev(fmrx_channels *c, float *d_audio_f32, int16_t *d_pcm16, int pcm_policy, void *stream)
{
    if (!c) return fail(FMRX_EINVAL, "channels_process_dev: null handle");
    FMRX_HIP(hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!c->de.on) return bank_process_dev(c->bank.get(), d_audio_f32, d_pcm16, pcm_policy, s);
    // de-emphasis: the bank writes the handle's f32 rows; behind it (its internal streams have joined s) the pass writes the caller's
    FMRX_TRY(bank_process_dev(c->bank.get(), c->de.in.p, nullptr, pcm_policy, s));
    return c->de.run(c->n_audio, d_audio_f32, d_pcm16, c->audio_channels, pcm_policy, c->opt, false, s);
}

int fmrx_channels_set_deemphasis(fmrx_channels *c, double tau_us)
{
    if (!c) return fail(FMRX_EINVAL, "channels_set_deemphasis: null handle");
    FMRX_HIP(hipSetDevice(c->device));
    return c->de.set(static_cast<double>(c->p.audio_Fs), tau_us, static_cast<size_t>(c->n_channels) * c->audio_channels, c->n_audio, c->opt);
}

int fmrx_channels_deemph_diagnostics(fmrx_channels *c, unsigned long long *segments, unsigned long long *missed)
{
    if (!c) return fail(FMRX_EINVAL, "channels_deemph_diagnostics: null handle");
    FMRX_HIP(hipSetDevice(c->device));
    return c->de.diagnostics(segments, missed);
}

int fmrx_channels_load_dev(fmrx_channels *c, const uint8_t *d_iq, void *stream)
{
    if (!c || !d_iq) return fail(FMRX_EINVAL, "channels_load_dev: null argument");
    FMRX_HIP(hipSetDevice(c->device));
    return load_slots(c, d_iq, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
}

int fmrx_channels_process(fmrx_channels *c, const uint8_t *iq, float *audio_f32, int16_t *pcm16, int pcm_policy)
{
    if (!c || !iq) return fail(FMRX_EINVAL, "channels_process: null argument");
    FMRX_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    FMRX_TRY(load_slots(c, iq, hipMemcpyHostToDevice, s));
    FMRX_TRY(fmrx_channels_process_dev(c, audio_f32 ? c->f32_out.p : nullptr, pcm16 ? c->pcm_out.p : nullptr, pcm_policy, s));
    const size_t n = c->n_audio * c->n_channels * c->audio_channels;
    if (audio_f32) FMRX_HIP(hipMemcpyAsync(audio_f32, c->f32_out.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (pcm16) FMRX_HIP(hipMemcpyAsync(pcm16, c->pcm_out.p, n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipStreamSynchronize(s));
    return FMRX_OK;
}

int fmrx_channels_read_tap(fmrx_channels *c, int channel, int which, float *out, size_t *n)
{
    if (!c || !n) return fail(FMRX_EINVAL, "channels_read_tap: null argument");
    FMRX_HIP(hipSetDevice(c->device));
    return bank_read_tap(c->bank.get(), channel, which, out, n);
}

}  // extern "C"
