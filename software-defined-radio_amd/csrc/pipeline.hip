// pipeline.hip -- the receiver pipeline handle of include/fmrx.h.
//
// Replaces main()'s setup and the three thread bodies of the reference:
//   RF_FrontEnd  src/project.cpp:40-152   (u8 -> IF I/Q -> FM demod)
//   RF_MONO      src/project.cpp:311-382  (audio FIR + decimate | resample)
//   RF_STEREO    src/project.cpp:154-309  (all-pass, pilot/stereo BPFs, PLL,
//                                          mixer, second audio FIR, L/R)
// with every intermediate resident in HBM and the carried state
// (src/project.cpp:61-65, 446-458) owned by the handle.  The producer/consumer
// queue of the reference (project.cpp:470-496) has no counterpart here: stages
// are kernels on one HIP stream, so the hand-off is stream order.
//
// Device layout of one block (n = complex input samples, n_if = n/rf_decim):
//   in      u8   [2n]                         raw I/Q (host-buffer entry point only; process_dev reads the caller's)
//   fe_hist u8   [hist_bytes] x2              the stream's last bytes (= I_state/Q_state), ping-pong
//   ifb     f32  [2 n_if]                     interleaved IF I,Q -- only with set_keep_intermediates / generic path
//   demod   f32  [Hd | n_if] x2               discriminator output; the previous block's tail is the history
//   mono    f32  [n_audio]                    (mono modes 0/1 write straight into the caller's buffers)
//   stereo: carrier, bpf [n_if]; pll [n_if+1]; mixer [Hm | n_if]; final, L, R [n_audio]
// The all-pass delay of the stereo path (project.cpp:194, filter.cpp:14-29) is
// not a kernel: the mono audio FIR simply reads demod `delay` samples earlier.
#include "fmrx_internal.hpp"

using namespace fmrx;

struct fmrx_pipeline {
    fmrx_params p{};
    int channels = 1;
    int device = 0;
    size_t max_bytes = 0;
    bool resample = false;
    bool force_generic = false;
    bool profiling = false;
    int prof_every = 1;           // HIP events around every prof_every-th call
    unsigned long seq = 0;        // calls since profiling was enabled
    int Ha = 0;     // audio-stage history, in its input samples
    int delay = 0;  // all-pass delay (stereo), samples
    int Hd = 0;     // history kept in front of demod (>= what the stages need, multiple of 4: keeps demod[0] 16-byte aligned)
    int Hm = 0;     // history kept in front of the stereo mixer output (same rule)
    int St = 0;     // stereo taps
    bool keep_if = false;        // materialise the IF I/Q stream (diagnostics / read_tap)
    bool prev_override = false;  // the next block takes IF[-1] from prev_iq (after set_state)
    bool if_valid = false;       // ifb holds the last block's IF samples
    bool demod_valid = true;     // the demod buffer holds the whole last block (not just its tail: fused mono kernel)
    bool mixer_valid = false;    // the mixer output of the last block was stored (the fused stereo kernel keeps it on chip)
    bool pll_warm = false;       // the PLL has seen a block since reset / set_state (its state is a locked one)
    double pll_off = 0.0;        // host copy of the PLL's trigOffset (IF samples since the stream began, as the reference counts them)
    Options opt;                 // copied from the process defaults at creation; fmrx_pipeline_set_option

    hipStream_t stream = nullptr;  // used by the host-buffer entry point
    FePlan fe;
    AudioPlan audio;
    ResamplePlan rs;           // resampler (modes 2, 3)
    BpfPairPlan bpf_plan;      // stereo + pilot band-pass filters

    DevBuf<uint8_t> in;
    DevBuf<uint8_t> fe_hist[2];
    int fe_cur = 0;
    DevBuf<float> prev_iq[2];
    int prev_cur = 0;
    DevBuf<float> ifb, mono;
    // discriminator output, two buffers [Hd | n_if] used alternately: the history of a block is the
    // tail of the previous block's buffer, so nothing has to be copied between blocks unless a kernel
    // needs it contiguous in front of its input (materialise_history)
    DevBuf<float> demod_buf[2];
    int demod_last = 0;          // buffer that holds the last processed block
    size_t demod_n_last = 0;     // its length; its history front is valid iff demod_front[demod_last]
    bool demod_front[2] = {true, true};
    DevBuf<float> pll_state, pll_scratch, mixer, st_final, left, right;
    // the stereo intermediates a call writes: set[0] always, except under option overlap_calls (stereo, modes 0/1, parallel
    // PLL), where the three stages of a call run on internal streams, a call apart each -- front (front end, band-pass pair,
    // the PLL's chunk records), PLL (lanes + repair), output stage -- on the set of the call's parity; the caller's stream
    // waits for the output stage's event
    struct StereoSet {
        DevBuf<float> carrier, bpf, pll;
    } set[2];
    int last_set = 0;                // set the last call used (read_tap)
    DevBuf<float> lti_rec[2];
    hipStream_t ov_stream[3] = {};   // front, PLL, output
    hipEvent_t ov_done[3][2] = {};   // [stage][parity]: the stage of the last call of that parity has finished
    hipEvent_t ov_entry = nullptr;   // the caller's stream at the call: what it did with the previous output is over
    bool ov_ready = false;           // overlap_setup has completed
    int ov_active = 0;               // the regime (option value) of the last call
    // state_stereofilt: the mixer output's last Hm samples (index Hm+g holds sample g < 0), written by one call
    // and read by the next: two buffers used alternately, mix_cur = the one the next call reads
    DevBuf<float> mix_tail[2];
    int mix_cur = 0;
    DevBuf<float> out_f32;
    DevBuf<int16_t> out_pcm;
    // de-emphasis (kernels_deemph.hip; off by default): while it is on, the producing stage of a call writes f32 into de.in
    // ([channels][n_audio]) instead of the caller's buffers and no PCM; one pass behind it writes the caller's
    Deemph de;
    // asynchronous host-buffer calls (fmrx_pipeline_submit / _wait): two slots, each with its own stream and device staging
    // buffers (slot 0 = `stream`, `in`, `out_f32`, `out_pcm` above): block i+1's copy to the device runs under block i's kernels
    // and block i-1's copy back.  Only the kernels of consecutive blocks are ordered (they carry the state): ev_kern.
    hipStream_t stream2 = nullptr;
    DevBuf<uint8_t> in2;
    DevBuf<float> out_f32_2;
    DevBuf<int16_t> out_pcm_2;
    hipEvent_t ev_kern[2] = {}, ev_done[2] = {};
    bool slot_busy[2] = {false, false};
    int next_slot = 0, oldest_slot = 0, last_kern_slot = -1;
    bool async_ready = false;

    size_t last_n_if = 0, last_n_audio = 0;
    const float *last_mono = nullptr;   // where the last block's mono audio was written
    // profiling: a ring of per-call event quadruples {start, after FE kernel,
    // after audio stage, end}, recorded on the caller's stream
    static constexpr int kRing = 128;
    hipEvent_t ev[kRing][4] = {};
    unsigned long calls = 0;      // profiled calls since profiling was enabled

    ~fmrx_pipeline()
    {
        for (hipStream_t st : {stream, stream2, ov_stream[0], ov_stream[1], ov_stream[2]})
            if (st) {
                (void)hipStreamSynchronize(st);
                (void)hipStreamDestroy(st);
            }
        for (auto &q : ev)
            for (auto &e : q)
                if (e) (void)hipEventDestroy(e);
        for (auto &q : ov_done)
            for (auto &e : q)
                if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_kern[0], ev_kern[1], ev_done[0], ev_done[1], ov_entry})
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

__global__ void hist_update_kernel(const uint8_t *__restrict__ old_hist, const uint8_t *__restrict__ x, long n_bytes,
                                   int hb, uint8_t *__restrict__ new_hist)
{
    // new history = last hb bytes of the stream [old_hist | x]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hb) return;
    const long src = static_cast<long>(i) + n_bytes - hb;  // offset into x; negative -> old history
    new_hist[i] = src >= 0 ? x[src] : old_hist[hb + src];
}

// The fused mono kernel gives each wave whole batches of 256 audio samples; below opt.fused_min_audio
// (default 65 536) audio samples per call there are too few batches to fill the chip and the two-kernel
// path is used (0 = always fuse when possible, a huge value = never).

int n_if_of(const fmrx_pipeline *pl, size_t n_bytes) { return static_cast<int>((n_bytes / 2) / pl->p.rf_decim); }

size_t n_audio_of(const fmrx_pipeline *pl, size_t n_bytes)
{
    const size_t n_if = (n_bytes / 2) / pl->p.rf_decim;
    if (pl->resample) return (n_if * static_cast<size_t>(pl->p.audio_upsamp)) / pl->p.audio_decim;
    return n_if / pl->p.audio_decim;
}

// resample_launch's margins hold for [d_x - delay, + n_in) iff it lies that far inside one of the discriminator buffers
// ([Hd | n_if | margin], finite throughout); checked against the allocations, not assumed
bool resample_margins(const fmrx_pipeline *pl, const float *d_x, size_t n_in, int delay)
{
    for (int i = 0; i < 2; i++) {
        const float *b = pl->demod_buf[i].p, *e = b + pl->demod_buf[i].n;
        if (b && d_x - delay - kResampleFront >= b && d_x - delay + n_in + kResampleBack <= e) return true;
    }
    return false;
}

int audio_stage(fmrx_pipeline *pl, const float *d_x, size_t n_in, int delay, float *d_y, hipStream_t s)
{
    if (pl->resample)
        return resample_launch(pl->rs, d_x, n_in, delay, d_y, pl->opt, s, pl->force_generic, false, nullptr, 0,
                               resample_margins(pl, d_x, n_in, delay));
    return audio_fir_launch(pl->audio, d_x, nullptr, n_in, delay, d_y, nullptr, 0, s, pl->force_generic);
}


int reset_state(fmrx_pipeline *pl)
{
    pl->slot_busy[0] = pl->slot_busy[1] = false;   // the device-wide wait below retires whatever was submitted
    pl->next_slot = pl->oldest_slot = 0;
    pl->last_kern_slot = -1;
    // process_dev runs on the caller's stream: whatever is still in flight there must not see the
    // state change under it (reset is rare; a device-wide wait is the simple, safe order)
    FMRX_HIP(hipDeviceSynchronize());
    hipStream_t s = pl->stream;
    for (int i = 0; i < 2; i++) {
        FMRX_TRY(k_fill_u8(pl->fe_hist[i].p, pl->fe.hist_bytes, 128, s));
        FMRX_HIP(hipMemsetAsync(pl->prev_iq[i].p, 0, 2 * sizeof(float), s));
    }
    for (int i = 0; i < 2; i++) FMRX_HIP(hipMemsetAsync(pl->demod_buf[i].p, 0, pl->Hd * sizeof(float), s));
    pl->demod_last = 0;
    pl->demod_n_last = 0;
    pl->demod_front[0] = pl->demod_front[1] = true;
    if (pl->channels == 2) {
        for (int i = 0; i < 2; i++) FMRX_HIP(hipMemsetAsync(pl->mix_tail[i].p, 0, pl->Hm * sizeof(float), s));
        const float init[6] = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f};  // src/project.cpp:458
        FMRX_HIP(hipMemcpyAsync(pl->pll_state.p, init, sizeof(init), hipMemcpyHostToDevice, s));
        FMRX_HIP(hipMemsetAsync(pl->pll_scratch.p + 5, 0, 3 * sizeof(float), s));   // no phase-slope history yet
    }
    FMRX_TRY(pl->de.reset(0, pl->channels, s));
    FMRX_HIP(hipStreamSynchronize(s));
    pl->fe_cur = pl->prev_cur = pl->mix_cur = 0;
    pl->prev_override = false;
    pl->if_valid = false;
    pl->pll_warm = false;
    pl->pll_off = 0.0;
    return FMRX_OK;
}

int check_block(const fmrx_pipeline *pl, size_t n_bytes)
{
    const fmrx_params &p = pl->p;
    if (n_bytes == 0 || n_bytes % 2) return fail(FMRX_EINVAL, "process: n_bytes %zu must be a positive even number", n_bytes);
    if (n_bytes > pl->max_bytes) return fail(FMRX_EINVAL, "process: block of %zu bytes exceeds max_block_bytes %zu", n_bytes, pl->max_bytes);
    const size_t n = n_bytes / 2;
    if (n % p.rf_decim) return fail(FMRX_EINVAL, "process: %zu samples not a multiple of rf_decim %d", n, p.rf_decim);
    if (n < static_cast<size_t>(p.rf_taps - 1)) return fail(FMRX_EINVAL, "process: %zu samples < rf_taps-1", n);
    const size_t n_if = n / p.rf_decim;
    if (pl->resample) {
        if ((n_if * p.audio_upsamp) % p.audio_decim)
            return fail(FMRX_EINVAL, "process: n_if*upsamp = %zu not a multiple of audio_decim %d", n_if * p.audio_upsamp, p.audio_decim);
    } else if (n_if % p.audio_decim) {
        return fail(FMRX_EINVAL, "process: %zu IF samples not a multiple of audio_decim %d", n_if, p.audio_decim);
    }
    if (n_if < static_cast<size_t>(pl->Ha)) return fail(FMRX_EINVAL, "process: %zu IF samples < audio history %d", n_if, pl->Ha);
    if (pl->channels == 2 && n_if < static_cast<size_t>(pl->St - 1))
        return fail(FMRX_EINVAL, "process: %zu IF samples < stereo_taps-1", n_if);
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_pipeline_create(fmrx_pipeline **out, const fmrx_params *p, int channels, size_t max_block_bytes, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "pipeline_create: null argument");
    if (channels != 1 && channels != 2) return fail(FMRX_EINVAL, "pipeline_create: channels must be 1 or 2");
    if (p->rf_taps < 2 || p->rf_taps > 65535 || p->audio_taps < 2 || p->audio_taps > 65535 || p->rf_decim < 1 ||
        p->audio_decim < 1 || p->audio_upsamp < 0)
        return fail(FMRX_EINVAL, "pipeline_create: bad parameters");
    if (channels == 2 && (p->stereo_taps < 2 || p->stereo_taps > 65535))
        return fail(FMRX_EINVAL, "pipeline_create: bad stereo_taps");
    if (max_block_bytes < 2) return fail(FMRX_EINVAL, "pipeline_create: max_block_bytes too small");
    // the reference's resampler refreshes its state in steps of upsamp from slot upsamp-1 (src/filter.cpp:218-222) and reads
    // it at taps-1 - d*upsamp (:207): the two meet only when upsamp divides taps.  Otherwise the reference is not a stream (its
    // output depends on where the blocks are cut), and the stream this handle computes would differ from it silently
    if (p->audio_upsamp > 0 && p->audio_taps % p->audio_upsamp != 0)
        return fail(FMRX_EINVAL, "pipeline_create: audio_taps %d is not a multiple of audio_upsamp %d", p->audio_taps, p->audio_upsamp);
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));

    fmrx_pipeline *pl = new fmrx_pipeline;
    pl->opt = options_snapshot();
    pl->p = *p;
    pl->channels = channels;
    pl->device = device;
    pl->max_bytes = max_block_bytes;
    pl->resample = p->audio_upsamp > 0;
    pl->Ha = pl->resample ? (p->audio_taps - 1) / p->audio_upsamp : p->audio_taps - 1;
    pl->St = channels == 2 ? p->stereo_taps : 0;
    pl->delay = channels == 2 ? (p->stereo_taps - 1) / 2 : 0;
    pl->Hd = pl->Ha + pl->delay;
    if (channels == 2 && pl->St - 1 + 3 > pl->Hd) pl->Hd = pl->St - 1 + 3;   // the band-pass pair kernel reads 16-byte chunks
    if (pl->resample) pl->Hd += kResampleFront;   // the matrix-core resampler stages whole 16-byte pieces around its windows
    pl->Hd = (pl->Hd + 3) / 4 * 4 + 4;   // the specialised audio kernel loads aligned 16-byte chunks
    pl->Hm = (pl->Ha + 3) / 4 * 4 + 4;

    int rc = FMRX_OK;
    auto body = [&]() -> int {
        FMRX_HIP(hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking));
        for (auto &q : pl->ev)
            for (auto &e : q) FMRX_HIP(hipEventCreate(&e));
        const Filters f = design_filters(*p, channels == 2);
        FMRX_TRY(fe_plan_init(pl->fe, f.rf.data(), p->rf_taps, p->rf_decim));
        if (pl->resample) {
            FMRX_TRY(resample_plan_init(pl->rs, f.audio.data(), p->audio_taps, p->audio_decim, p->audio_upsamp));
        } else {
            FMRX_TRY(audio_plan_init(pl->audio, f.audio.data(), p->audio_taps, p->audio_decim));
        }
        const size_t n_max = max_block_bytes / 2;
        const size_t n_if = n_max / p->rf_decim;
        const size_t n_au = n_audio_of(pl, max_block_bytes) + 1;
        FMRX_TRY(pl->in.alloc(pl->fe.hist_bytes + max_block_bytes + 16));
        for (int i = 0; i < 2; i++) {
            FMRX_TRY(pl->fe_hist[i].alloc(pl->fe.hist_bytes));
            FMRX_TRY(pl->prev_iq[i].alloc(2));
        }
        FMRX_TRY(pl->ifb.alloc(2 * n_if + 16));
        for (int i = 0; i < 2; i++) {   // [Hd | n_if | margin]: all of it finite from the start (resample_launch's margins)
            FMRX_TRY(pl->demod_buf[i].alloc(pl->Hd + n_if + 16 + kResampleBack));
            FMRX_HIP(hipMemset(pl->demod_buf[i].p, 0, (pl->Hd + n_if + 16 + kResampleBack) * sizeof(float)));
        }
        FMRX_TRY(pl->mono.alloc(n_au));
        if (channels == 2) {
            FMRX_TRY(bpf_pair_plan_init(pl->bpf_plan, f.stereo.data(), f.pilot.data(), p->stereo_taps));
            FMRX_TRY(pl->set[0].carrier.alloc(n_if + 16));
            FMRX_TRY(pl->set[0].bpf.alloc(n_if + 16));
            FMRX_TRY(pl->set[0].pll.alloc(n_if + 17));
            FMRX_TRY(pl->pll_state.alloc(8));
            FMRX_TRY(pl->pll_scratch.alloc(pll_parallel_scratch_floats(n_if)));
            FMRX_HIP(hipMemset(pl->pll_scratch.p, 0, 8 * sizeof(float)));
            FMRX_TRY(pl->mixer.alloc(pl->Hm + n_if + 16));
            for (int i = 0; i < 2; i++) FMRX_TRY(pl->mix_tail[i].alloc(pl->Hm + 4));
            FMRX_TRY(pl->st_final.alloc(n_au));
            FMRX_TRY(pl->left.alloc(n_au));
            FMRX_TRY(pl->right.alloc(n_au));
        }
        FMRX_TRY(pl->out_f32.alloc(2 * n_au));
        FMRX_TRY(pl->out_pcm.alloc(2 * n_au));
        return reset_state(pl);
    };
    rc = body();
    if (rc != FMRX_OK) {
        fmrx_pipeline_destroy(pl);
        return rc;
    }
    *out = pl;
    return FMRX_OK;
}

int fmrx_pipeline_destroy(fmrx_pipeline *pl)
{
    if (!pl) return FMRX_OK;
    (void)hipSetDevice(pl->device);
    delete pl;
    return FMRX_OK;
}

int fmrx_pipeline_reset(fmrx_pipeline *pl)
{
    if (!pl) return fail(FMRX_EINVAL, "pipeline_reset: null handle");
    FMRX_HIP(hipSetDevice(pl->device));
    return reset_state(pl);
}

size_t fmrx_pipeline_n_if(const fmrx_pipeline *pl, size_t n_bytes) { return pl ? n_if_of(pl, n_bytes) : 0; }
size_t fmrx_pipeline_n_audio(const fmrx_pipeline *pl, size_t n_bytes) { return pl ? n_audio_of(pl, n_bytes) : 0; }

int fmrx_pipeline_set_profiling(fmrx_pipeline *pl, int on)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    pl->profiling = on != 0;
    pl->prof_every = on > 1 ? on : 1;
    pl->seq = 0;
    pl->calls = 0;
    return FMRX_OK;
}

int fmrx_pipeline_pll_diagnostics(fmrx_pipeline *pl, unsigned *repaired_segments, float *max_dphase, float *max_dinteg)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    if (pl->channels != 2) return fail(FMRX_EINVAL, "pll_diagnostics: not a stereo pipeline");
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_HIP(hipDeviceSynchronize());
    unsigned hdr[8];
    FMRX_HIP(hipMemcpy(hdr, pl->pll_scratch.p, sizeof(hdr), hipMemcpyDeviceToHost));
    if (repaired_segments) *repaired_segments = hdr[2];
    if (max_dphase) std::memcpy(max_dphase, &hdr[3], sizeof(float));
    if (max_dinteg) std::memcpy(max_dinteg, &hdr[4], sizeof(float));
    return FMRX_OK;
}

int fmrx_pipeline_set_option(fmrx_pipeline *pl, const char *name, long value)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    return set_option_in(pl->opt, name, value);
}

int fmrx_pipeline_set_deemphasis(fmrx_pipeline *pl, double tau_us)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    FMRX_HIP(hipSetDevice(pl->device));
    return pl->de.set(static_cast<double>(pl->p.audio_Fs), tau_us, pl->channels, n_audio_of(pl, pl->max_bytes) + 1, pl->opt);
}

int fmrx_pipeline_deemph_diagnostics(fmrx_pipeline *pl, unsigned long long *segments, unsigned long long *missed)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    FMRX_HIP(hipSetDevice(pl->device));
    return pl->de.diagnostics(segments, missed);
}

int fmrx_pipeline_set_keep_intermediates(fmrx_pipeline *pl, int on)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    pl->keep_if = on != 0;
    return FMRX_OK;
}

int fmrx_pipeline_set_force_generic(fmrx_pipeline *pl, int on)
{
    if (!pl) return fail(FMRX_EINVAL, "null handle");
    pl->force_generic = on != 0;
    return FMRX_OK;
}

// internal streams, events and the second buffer set of option overlap_calls, on first use
static int overlap_setup(fmrx_pipeline *pl)
{
    if (pl->ov_ready) return FMRX_OK;
    // every handle is created only where it is still missing: a call that failed half way (out of memory, say) is simply
    // continued by the next one, nothing is created twice and nothing leaks (destroy frees whatever exists)
    const size_t n_if = (pl->max_bytes / 2) / pl->p.rf_decim;
    FMRX_TRY(pl->set[1].carrier.ensure(pl->set[0].carrier.n));
    FMRX_TRY(pl->set[1].bpf.ensure(pl->set[0].bpf.n));
    FMRX_TRY(pl->set[1].pll.ensure(pl->set[0].pll.n));
    for (auto &b : pl->lti_rec) FMRX_TRY(b.ensure(pll_parallel_lti_floats(n_if) + 2));
    for (auto &q : pl->ov_done)
        for (auto &e : q)
            if (!e) FMRX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!pl->ov_entry) FMRX_HIP(hipEventCreateWithFlags(&pl->ov_entry, hipEventDisableTiming));
    for (auto &st : pl->ov_stream)
        if (!st) FMRX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    pl->ov_ready = true;
    return FMRX_OK;
}

// ---- one process call, in stages ----------------------------------------------------------
// What the stages of one call share: the caller's arguments, then what call_setup derives from them
struct Call {
    const uint8_t *iq;
    size_t n_bytes;
    float *audio_f32;            // the caller's outputs (either may be null)
    int16_t *pcm16;
    int pcm_policy;
    hipStream_t s;               // the caller's stream
    hipStream_t sf, sp, so;      // front (front end, band-pass pair), PLL, stereo output stage: s but under overlap_calls
    size_t n, n_if, n_au;
    int cur;                     // this block's discriminator buffer (the other one holds the last block's); overlap parity
    float *dbuf, *demod;         // that buffer [Hd | n_if], and its block region
    const float *hist_end;       // one past the previous block's last discriminator sample
    const uint8_t *hist;         // the front end's byte history and IF[-1]; *_next: where the next block's go
    uint8_t *hist_next;
    const float *prev;
    float *prev_next;
    bool keep_if;                // the IF stream is materialised
    bool ovl;                    // option overlap_calls applies
    bool fused;                  // the fused mono kernel does the whole call
    bool prof;                   // the call records the event quadruple ev
    hipEvent_t *ev;
    // de-emphasis on: audio_f32 above is the handle's own rows and pcm16 null; these are the caller's
    bool de;
    float *user_f32;
    int16_t *user_pcm;
};

// profiling: event k of the call's quadruple {start, after the front end, after the audio stage, end}, on the caller's stream
static int mark(const Call &c, int k)
{
    if (c.prof) FMRX_HIP(hipEventRecord(c.ev[k], c.s));
    return FMRX_OK;
}

// for kernels that index history at negative offsets of their input
static int materialise_history(fmrx_pipeline *pl, const Call &c)
{
    FMRX_HIP(hipMemcpyAsync(c.dbuf, c.hist_end - pl->Hd, pl->Hd * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    pl->demod_front[c.cur] = true;
    return FMRX_OK;
}

// after the front end: the next block's IF[-1], byte history (unless the front-end kernel wrote it: hist_done) and
// discriminator history are this block's
static int advance_state(fmrx_pipeline *pl, const Call &c, bool hist_done)
{
    pl->prev_cur ^= 1;
    pl->prev_override = false;
    pl->fe_cur ^= 1;
    const int hb = pl->fe.hist_bytes;
    if (!hist_done) {
        hipLaunchKernelGGL(hist_update_kernel, dim3((hb + 255) / 256), dim3(256), 0, c.sf, c.hist, c.iq,
                           static_cast<long>(c.n_bytes), hb, c.hist_next);
        FMRX_LAUNCH_CHECK("hist_update_kernel");
    }
    pl->demod_last = c.cur;
    pl->demod_n_last = c.n_if;
    return FMRX_OK;
}

static int call_setup(fmrx_pipeline *pl, Call &c)
{
    const fmrx_params &p = pl->p;
    c.sf = c.sp = c.so = c.s;
    c.n = c.n_bytes / 2;
    c.n_if = c.n / p.rf_decim;
    c.n_au = n_audio_of(pl, c.n_bytes);
    pl->last_n_if = c.n_if;
    pl->last_n_audio = c.n_au;
    // this block's discriminator output goes to the buffer the previous block did not use
    c.cur = pl->demod_last ^ 1;
    c.dbuf = pl->demod_buf[c.cur].p;
    c.demod = c.dbuf + pl->Hd;
    c.hist_end = pl->demod_buf[pl->demod_last].p + pl->Hd + pl->demod_n_last;
    pl->demod_front[c.cur] = false;
    c.hist = pl->fe_hist[pl->fe_cur].p;
    c.hist_next = pl->fe_hist[pl->fe_cur ^ 1].p;
    c.prev = pl->prev_iq[pl->prev_cur].p;
    c.prev_next = pl->prev_iq[pl->prev_cur ^ 1].p;
    // events around every prof_every-th call: a record costs ~5 us of stream time
    c.prof = pl->profiling && (pl->seq++ % static_cast<unsigned long>(pl->prof_every) == 0);
    c.ev = pl->ev[pl->calls % fmrx_pipeline::kRing];
    FMRX_TRY(mark(c, 0));
    const bool mfma = pl->opt.fe_variant == 0;
    // option demod = 1: the model's arctangent demodulator on the IF stream (materialised for it), instead of the front-end kernels' own discriminator
    c.keep_if = pl->keep_if || pl->opt.demod == 1;
    // option overlap_calls: front | PLL | output stage of the stereo chain of consecutive calls on internal streams (see the struct)
    c.ovl = pl->opt.overlap_calls != 0 && pl->channels == 2 && !pl->resample && !pl->force_generic && !c.keep_if &&
            !pl->profiling && pl->opt.pll_mode == 0 && mfma && c.n_if >= static_cast<size_t>(pl->Hd) &&
            fe_mfma_available(pl->fe, c.iq, c.n, c.hist) && stereo_out_available(p.audio_taps, p.audio_decim);
    c.fused = pl->channels == 1 && !pl->resample && !pl->force_generic && !c.keep_if && mfma &&
              c.n_if >= static_cast<size_t>(pl->Hd) && static_cast<long>(c.n_au) >= pl->opt.fused_min_audio &&
              mono_fused_available(pl->fe, pl->audio, c.iq, c.n, c.hist);
    return FMRX_OK;
}

static int overlap_begin(fmrx_pipeline *pl, Call &c)
{
    const int regime = c.ovl ? pl->opt.overlap_calls : 0;
    if (regime != pl->ov_active) {   // change of regime between calls: everything in flight first
        FMRX_HIP(hipDeviceSynchronize());
        pl->ov_active = regime;
    }
    if (c.ovl) FMRX_TRY(overlap_setup(pl));
    pl->last_set = c.ovl ? c.cur : 0;
    if (!c.ovl) return FMRX_OK;
    // overlap_calls 1: the front on an internal stream, PLL and output stage on the caller's (fewest event operations: at these
    // step sizes the host's enqueue rate is the next limit); 2: all three on internal streams
    c.sf = pl->ov_stream[0];
    if (pl->opt.overlap_calls >= 2) {
        c.sp = pl->ov_stream[1];
        c.so = pl->ov_stream[2];
    }
    // the front writes this parity's buffers: the last call of the same parity must be through with them; the output
    // stage writes the caller's buffers: whatever the caller's stream still does with them comes first (the input is the
    // one thing the option vouches for)
    FMRX_HIP(hipStreamWaitEvent(c.sf, pl->ov_done[2][c.cur], 0));
    if (c.so != c.s) {
        FMRX_HIP(hipEventRecord(pl->ov_entry, c.s));
        FMRX_HIP(hipStreamWaitEvent(c.so, pl->ov_entry, 0));
    }
    return FMRX_OK;
}

// de-emphasis on: the stages below write f32 rows of the handle's own and no PCM (every stage already serves such a caller)
static void deemph_redirect(fmrx_pipeline *pl, Call &c)
{
    c.de = pl->de.on;
    if (!c.de) return;
    c.user_f32 = c.audio_f32;
    c.user_pcm = c.pcm16;
    c.audio_f32 = pl->de.in.p;
    c.pcm16 = nullptr;
}

// ... and this pass writes the caller's buffers, on the stream of the stage that wrote the rows
static int deemph_stage(fmrx_pipeline *pl, const Call &c, hipStream_t s)
{
    return pl->de.run(c.n_au, c.user_f32, c.user_pcm, pl->channels, c.pcm_policy, pl->opt, pl->force_generic, s);
}

// ---- RF_FrontEnd + RF_MONO of modes 0/1 in one kernel (kernels_fe_mfma.hip): the discriminator output stays on chip;
//      only its tail (state_mono) is written for the next block ----
static int fused_mono(fmrx_pipeline *pl, const Call &c)
{
    const bool hist_done = c.n_bytes >= static_cast<size_t>(pl->fe.hist_bytes);
    // f32 audio is written only where somebody will read it: the caller's buffer, or the handle's own when
    // no PCM was asked for either (read_tap); PCM-only callers get the reference's output format and nothing else
    float *dst = c.audio_f32 ? c.audio_f32 : (c.pcm16 ? nullptr : pl->mono.p);
    FMRX_TRY(mono_fused_launch(pl->fe, pl->audio, c.iq, c.n, c.hist, c.prev, c.hist_end, c.demod, pl->Hd, c.prev_next, dst,
                               c.pcm16, c.pcm_policy, hist_done ? c.hist_next : nullptr, pl->opt, c.s));
    pl->if_valid = false;
    pl->demod_valid = false;
    pl->last_mono = dst;
    FMRX_TRY(mark(c, 1));
    FMRX_TRY(advance_state(pl, c, hist_done));
    return mark(c, 2);
}

// ---- RF_FrontEnd: project.cpp:82-128 (u8 -> IF I/Q -> discriminator) ----
static int front_end(fmrx_pipeline *pl, const Call &c)
{
    const int hb = pl->fe.hist_bytes;
    bool hist_done = false;
    pl->demod_valid = true;
    if (!pl->force_generic && pl->opt.fe_variant == 0 && fe_mfma_available(pl->fe, c.iq, c.n, c.hist)) {
        // matrix-core kernel: int8 MFMA FIR + discriminator, HBM-bound (kernels_fe_mfma.hip)
        hist_done = c.n_bytes >= static_cast<size_t>(hb);
        // everything but mono modes 0/1 reads the discriminator history at negative indices of this block's buffer:
        // the kernel copies it there itself (it is the tail of the previous block's buffer)
        const bool want_front = !(pl->channels == 1 && !pl->resample) && c.n_if >= static_cast<size_t>(pl->Hd);
        FMRX_TRY(fe_mfma_launch(pl->fe, c.iq, c.n, c.hist, pl->prev_override ? c.prev : nullptr, c.demod,
                                c.keep_if ? pl->ifb.p : nullptr, c.prev_next,
                                hist_done ? c.hist_next : nullptr, pl->opt, c.sf, want_front ? c.hist_end - pl->Hd : nullptr,
                                want_front ? c.dbuf : nullptr, pl->Hd));
        if (want_front) pl->demod_front[c.cur] = true;
        pl->if_valid = c.keep_if;
    } else if (!pl->force_generic && fe_fused_available(pl->fe, c.iq, c.n)) {
        // one kernel; the IF stream is written only when somebody asked to look at it, and the kernel
        // also leaves the stream's last bytes (I_state/Q_state, filter.cpp:182-187) for the next block
        hist_done = c.n_bytes >= static_cast<size_t>(hb);
        FMRX_TRY(fe_demod_launch(pl->fe, c.iq, c.n, c.hist, pl->prev_override ? c.prev : nullptr, c.demod,
                                 c.keep_if ? pl->ifb.p : nullptr, c.prev_next, hist_done ? c.hist_next : nullptr, pl->opt, c.s));
        pl->if_valid = c.keep_if;
    } else {
        FMRX_TRY(fe_launch(pl->fe, c.iq, c.n, c.hist, pl->ifb.p, pl->opt, c.s, pl->force_generic));
        FMRX_TRY(k_fm_demod_if(pl->ifb.p, c.n_if, c.prev, c.prev_next, c.demod, 0, c.s));
        pl->if_valid = true;
    }
    // fmDemodArctan (model/fmSupportLib.py:502-531) over the IF stream, IF[-1] = the carried prev_i / prev_q (their phase is the
    // model's state_phase modulo 2 pi; zeros at the start of a stream: atan2(0, 0) = 0 = the model's initial phase)
    if (pl->opt.demod == 1) FMRX_TRY(k_fm_demod_arctan_if(pl->ifb.p, c.n_if, c.prev, c.demod, c.s));
    FMRX_TRY(mark(c, 1));
    FMRX_TRY(advance_state(pl, c, hist_done));
    // a block shorter than the history keeps its own front valid, so that "tail of the previous
    // buffer" stays a contiguous Hd samples for whoever comes next
    if (c.n_if < static_cast<size_t>(pl->Hd)) FMRX_TRY(materialise_history(pl, c));
    return FMRX_OK;
}

// ---- outputs of the stages that write the handle's own buffers: f32 copies, PCM ----
static int write_outputs(const Call &c, const float *out_l, const float *out_r)
{
    if (c.audio_f32) {
        FMRX_HIP(hipMemcpyAsync(c.audio_f32, out_l, c.n_au * sizeof(float), hipMemcpyDeviceToDevice, c.s));
        if (out_r) FMRX_HIP(hipMemcpyAsync(c.audio_f32 + c.n_au, out_r, c.n_au * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    }
    if (c.pcm16) {
        if (out_r) FMRX_TRY(k_pcm16_stereo(out_l, out_r, c.n_au, c.pcm16, c.pcm_policy, c.s));
        else FMRX_TRY(k_pcm16(out_l, c.n_au, c.pcm16, c.pcm_policy, c.s));
    }
    return FMRX_OK;
}

static int mono_back_end(fmrx_pipeline *pl, const Call &c)
{
    if (!pl->resample) {
        // ---- RF_MONO, modes 0/1: audio FIR + decimate + PCM in one kernel (project.cpp:346;
        //      threadMonoOnly.cpp:185-191), straight into the caller's buffers ----
        float *dst = c.audio_f32 ? c.audio_f32 : pl->mono.p;
        const bool fast = audio_fast_available(pl->audio, c.demod) && !pl->force_generic;
        if (!fast && !pl->demod_front[c.cur]) FMRX_TRY(materialise_history(pl, c));
        FMRX_TRY(audio_fir_launch(pl->audio, c.demod, fast ? c.hist_end : nullptr, c.n_if, 0, dst, c.pcm16, c.pcm_policy, c.s,
                                  pl->force_generic));
        pl->last_mono = dst;
        return mark(c, 2);
    }
    // ---- RF_MONO, modes 2/3: rational resampler (project.cpp:353) ----
    if (!pl->demod_front[c.cur]) FMRX_TRY(materialise_history(pl, c));
    if (!pl->force_generic && resample_mfma_available(pl->rs, c.demod, c.n_if, 0, pl->opt)) {
        // the matrix-core kernel writes the caller's buffers itself; PCM-only callers get the reference's output
        // format and nothing else (as the fused mono kernel of modes 0/1)
        float *dst = c.audio_f32 ? c.audio_f32 : (c.pcm16 ? nullptr : pl->mono.p);
        FMRX_TRY(resample_launch(pl->rs, c.demod, c.n_if, 0, dst, pl->opt, c.s, false, false, c.pcm16, c.pcm_policy,
                                 resample_margins(pl, c.demod, c.n_if, 0)));
        pl->last_mono = dst;
        return mark(c, 2);
    }
    FMRX_TRY(audio_stage(pl, c.demod, c.n_if, 0, pl->mono.p, c.s));
    pl->last_mono = pl->mono.p;
    FMRX_TRY(mark(c, 2));
    return write_outputs(c, pl->mono.p, nullptr);
}

// fmPLL on the pilot band: the serial recurrence, or the parallel one (a stream's first block walks a serial head first);
// under overlap_calls the chunk records belong to the front, and events order the front, PLL and output streams
static int pll_stage(fmrx_pipeline *pl, const Call &c, fmrx_pipeline::StereoSet &b)
{
    const size_t n_if = c.n_if;
    const float fs = static_cast<float>(pl->p.if_Fs);
    if (pl->force_generic || pl->opt.pll_mode != 0) {
        // the serial recurrence: glibc's functions in the bit-exact mode (and pll_mode 2), fast math for pll_mode 1
        const int fast = !pl->force_generic && pl->opt.pll_mode == 1;
        FMRX_TRY(k_fm_pll(b.carrier.p, n_if, b.pll.p, pl->pll_state.p, 19e3f, fs, 2.0f, 0.0f, 0.01f, fast, c.s));
    } else {
        // a stream's first block starts unlocked: walk its first samples serially so that the
        // segment lanes extrapolate from a locked state; later blocks start locked already
        size_t head = 0;
        if (!pl->pll_warm) head = n_if < static_cast<size_t>(kPllHead) ? n_if : static_cast<size_t>(kPllHead);
        // what depends on the input alone (the linear system's chunk records) belongs to the front
        float *lti = c.ovl ? pl->lti_rec[c.cur].p : nullptr;
        if (c.ovl && n_if > head)
            FMRX_TRY(k_fm_pll_parallel(b.carrier.p + head, n_if - head, b.pll.p + head, pl->pll_state.p, 19e3f, fs, 2.0f, 0.0f,
                                       0.01f, pl->pll_scratch.p, pl->opt, c.sf, pl->pll_off + static_cast<double>(head), 1, lti));
        if (c.ovl) {   // read-after-write: the lanes read this call's carrier / chunk records, which the front wrote on its own stream
            FMRX_HIP(hipEventRecord(pl->ov_done[0][c.cur], c.sf));
            FMRX_HIP(hipStreamWaitEvent(c.sp, pl->ov_done[0][c.cur], 0));
        }
        if (head > 0)
            FMRX_TRY(k_fm_pll(b.carrier.p, head, b.pll.p, pl->pll_state.p, 19e3f, fs, 2.0f, 0.0f, 0.01f, 1, c.sp));
        if (n_if > head)
            FMRX_TRY(k_fm_pll_parallel(b.carrier.p + head, n_if - head, b.pll.p + head, pl->pll_state.p, 19e3f, fs, 2.0f, 0.0f,
                                       0.01f, pl->pll_scratch.p, pl->opt, c.sp, pl->pll_off + static_cast<double>(head),
                                       c.ovl ? 2 : 3, lti));
        pl->pll_warm = true;
        if (c.so != c.sp) {   // read-after-write: the output stage reads the NCO values and the PLL state the lanes / repair left
            FMRX_HIP(hipEventRecord(pl->ov_done[1][c.cur], c.sp));
            FMRX_HIP(hipStreamWaitEvent(c.so, pl->ov_done[1][c.cur], 0));
        }
    }
    pl->pll_off += static_cast<double>(n_if);
    return FMRX_OK;
}

// ---- RF_STEREO: project.cpp:194-280 ----
static int stereo_back_end(fmrx_pipeline *pl, const Call &c)
{
    const fmrx_params &p = pl->p;
    if (!pl->demod_front[c.cur]) FMRX_TRY(materialise_history(pl, c));
    pl->last_mono = pl->mono.p;
    fmrx_pipeline::StereoSet &b = pl->set[pl->last_set];
    const bool fused_out = !pl->resample && !pl->force_generic && stereo_out_available(p.audio_taps, p.audio_decim);
    float *mixer = pl->mixer.p + pl->Hm;
    if (!fused_out) FMRX_TRY(audio_stage(pl, c.demod, c.n_if, pl->delay, pl->mono.p, c.s));  // all-pass = index offset
    FMRX_TRY(mark(c, 2));
    FMRX_TRY(bpf_pair_launch(pl->bpf_plan, c.demod, c.n_if, b.bpf.p, b.carrier.p, c.sf, pl->force_generic));
    FMRX_TRY(pll_stage(pl, c, b));
    const float *tail_in = pl->mix_tail[pl->mix_cur].p;
    float *tail_out = pl->mix_tail[pl->mix_cur ^ 1].p;
    if (fused_out) {
        // mixer, both audio FIRs, L/R combine and PCM in one kernel, straight into the caller's buffers
        FMRX_TRY(stereo_out_launch(c.demod, b.bpf.p, b.pll.p, tail_in, tail_out, pl->Hm, c.n_if, pl->delay, pl->audio.h.p,
                                   p.audio_taps, p.audio_decim, pl->mono.p, pl->st_final.p,
                                   c.audio_f32 ? c.audio_f32 : (c.pcm16 ? nullptr : pl->left.p),
                                   c.audio_f32 ? c.audio_f32 + c.n_au : (c.pcm16 ? nullptr : pl->right.p), c.pcm16,
                                   c.pcm_policy, pl->keep_if ? mixer : nullptr, c.so));
        if (c.de && c.ovl) FMRX_TRY(deemph_stage(pl, c, c.so));   // in front of the event the caller's stream waits for
        if (c.ovl) {   // the caller's stream sees the call's output in its own order, as always
            FMRX_HIP(hipEventRecord(pl->ov_done[2][c.cur], c.so));
            if (c.so != c.s) FMRX_HIP(hipStreamWaitEvent(c.s, pl->ov_done[2][c.cur], 0));
        }
        pl->mixer_valid = pl->keep_if;
        pl->mix_cur ^= 1;
        return FMRX_OK;
    }
    FMRX_HIP(hipMemcpyAsync(pl->mixer.p, tail_in, pl->Hm * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    FMRX_TRY(k_mix(b.bpf.p, b.pll.p, c.n_if, mixer, c.s));
    FMRX_TRY(audio_stage(pl, mixer, c.n_if, 0, pl->st_final.p, c.s));
    FMRX_TRY(k_combine(pl->st_final.p, pl->mono.p, c.n_au, pl->left.p, pl->right.p, c.s));
    // the mixer output's last Hm samples (of [history | block]) are the next block's state_stereofilt
    FMRX_HIP(hipMemcpyAsync(tail_out, pl->mixer.p + c.n_if, pl->Hm * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    pl->mix_cur ^= 1;
    pl->mixer_valid = true;
    return write_outputs(c, pl->left.p, pl->right.p);
}

int fmrx_pipeline_process_dev(fmrx_pipeline *pl, const uint8_t *d_iq, size_t n_bytes, float *d_audio_f32,
                              int16_t *d_pcm16, int pcm_policy, void *stream)
{
    if (!pl || !d_iq) return fail(FMRX_EINVAL, "process_dev: null argument");
    FMRX_TRY(check_block(pl, n_bytes));
    FMRX_HIP(hipSetDevice(pl->device));   // the handle's buffers live there, whatever the caller's current device
    Call c{d_iq, n_bytes, d_audio_f32, d_pcm16, pcm_policy, static_cast<hipStream_t>(stream)};
    deemph_redirect(pl, c);
    FMRX_TRY(call_setup(pl, c));
    FMRX_TRY(overlap_begin(pl, c));
    if (c.fused) {
        FMRX_TRY(fused_mono(pl, c));
    } else {
        FMRX_TRY(front_end(pl, c));
        FMRX_TRY(pl->channels == 1 ? mono_back_end(pl, c) : stereo_back_end(pl, c));
    }
    if (c.de && !c.ovl) FMRX_TRY(deemph_stage(pl, c, c.s));
    FMRX_TRY(mark(c, 3));
    if (c.prof) pl->calls++;
    return FMRX_OK;
}

static int async_setup(fmrx_pipeline *pl)
{
    if (pl->async_ready) return FMRX_OK;
    const size_t n_au = n_audio_of(pl, pl->max_bytes) + 1;
    FMRX_TRY(pl->in2.ensure(pl->in.n));
    FMRX_TRY(pl->out_f32_2.ensure(2 * n_au));
    FMRX_TRY(pl->out_pcm_2.ensure(2 * n_au));
    if (!pl->stream2) FMRX_HIP(hipStreamCreateWithFlags(&pl->stream2, hipStreamNonBlocking));
    for (auto &e : pl->ev_kern)
        if (!e) FMRX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : pl->ev_done)
        if (!e) FMRX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    pl->async_ready = true;
    return FMRX_OK;
}

int fmrx_pipeline_wait(fmrx_pipeline *pl)
{
    if (!pl) return fail(FMRX_EINVAL, "wait: null handle");
    const int slot = pl->oldest_slot;
    if (!pl->slot_busy[slot]) return FMRX_OK;
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_HIP(hipEventSynchronize(pl->ev_done[slot]));
    pl->slot_busy[slot] = false;
    pl->oldest_slot = slot ^ 1;
    return FMRX_OK;
}

int fmrx_pipeline_submit(fmrx_pipeline *pl, const uint8_t *iq, size_t n_bytes, float *audio_f32, int16_t *pcm16, int pcm_policy)
{
    if (!pl || !iq) return fail(FMRX_EINVAL, "submit: null argument");
    FMRX_TRY(check_block(pl, n_bytes));
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_TRY(async_setup(pl));
    const int slot = pl->next_slot;
    if (pl->slot_busy[slot]) FMRX_TRY(fmrx_pipeline_wait(pl));   // two blocks in flight: the older one first
    hipStream_t s = slot ? pl->stream2 : pl->stream;
    uint8_t *d_in = slot ? pl->in2.p : pl->in.p;
    float *d_f32 = slot ? pl->out_f32_2.p : pl->out_f32.p;
    int16_t *d_pcm = slot ? pl->out_pcm_2.p : pl->out_pcm.p;
    const size_t n_au = n_audio_of(pl, n_bytes);
    const size_t nch = pl->channels;
    FMRX_HIP(hipMemcpyAsync(d_in, iq, n_bytes, hipMemcpyHostToDevice, s));
    // option overlap_calls vouches for inputs that are complete at the call; this one is still on its way: wait for it
    if (pl->opt.overlap_calls != 0) FMRX_HIP(hipStreamSynchronize(s));
    // the kernels of consecutive blocks carry the receiver's state: this block's follow the previous block's (the copies do not)
    if (pl->last_kern_slot >= 0 && pl->last_kern_slot != slot) FMRX_HIP(hipStreamWaitEvent(s, pl->ev_kern[pl->last_kern_slot], 0));
    FMRX_TRY(fmrx_pipeline_process_dev(pl, d_in, n_bytes, audio_f32 ? d_f32 : nullptr, pcm16 ? d_pcm : nullptr, pcm_policy, s));
    FMRX_HIP(hipEventRecord(pl->ev_kern[slot], s));
    pl->last_kern_slot = slot;
    if (audio_f32) FMRX_HIP(hipMemcpyAsync(audio_f32, d_f32, nch * n_au * sizeof(float), hipMemcpyDeviceToHost, s));
    if (pcm16) FMRX_HIP(hipMemcpyAsync(pcm16, d_pcm, nch * n_au * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipEventRecord(pl->ev_done[slot], s));
    pl->slot_busy[slot] = true;
    pl->next_slot = slot ^ 1;
    if (!pl->slot_busy[slot ^ 1]) pl->oldest_slot = slot;
    return FMRX_OK;
}

int fmrx_pipeline_process(fmrx_pipeline *pl, const uint8_t *iq, size_t n_bytes, float *audio_f32, int16_t *pcm16,
                          int pcm_policy)
{
    if (!pl || !iq) return fail(FMRX_EINVAL, "process: null argument");
    // the synchronous form = submit + wait for everything in flight (so mixing the two forms keeps the stream's order)
    FMRX_TRY(fmrx_pipeline_submit(pl, iq, n_bytes, audio_f32, pcm16, pcm_policy));
    FMRX_TRY(fmrx_pipeline_wait(pl));
    return fmrx_pipeline_wait(pl);
}

int fmrx_pipeline_read_tap(fmrx_pipeline *pl, int which, float *out, size_t *n)
{
    if (!pl || !n) return fail(FMRX_EINVAL, "read_tap: null argument");
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_HIP(hipDeviceSynchronize());
    const size_t n_if = pl->last_n_if, n_au = pl->last_n_audio;
    const float *src = nullptr;
    size_t cnt = 0;
    const bool st = pl->channels == 2;
    switch (which) {
    case FMRX_TAP_IF_I:
    case FMRX_TAP_IF_Q: cnt = n_if; break;
    case FMRX_TAP_DEMOD: src = pl->demod_buf[pl->demod_last].p + pl->Hd; cnt = n_if; break;   // the last block's region
    case FMRX_TAP_MONO:
        src = pl->last_mono; cnt = n_au;
        if (!src && out && cnt) return fail(FMRX_EINVAL, "read_tap: the last call wrote s16 PCM only (no f32 audio buffer was passed)");
        break;
    case FMRX_TAP_CARRIER: if (st) { src = pl->set[pl->last_set].carrier.p; cnt = n_if; } break;
    case FMRX_TAP_STEREO_BPF: if (st) { src = pl->set[pl->last_set].bpf.p; cnt = n_if; } break;
    case FMRX_TAP_PLL: if (st) { src = pl->set[pl->last_set].pll.p; cnt = n_if + 1; } break;
    case FMRX_TAP_MIXER:
        if (st) { src = pl->mixer.p + pl->Hm; cnt = n_if; }
        if (st && out && cnt && !pl->mixer_valid)
            return fail(FMRX_EINVAL, "read_tap: the fused stereo kernel keeps the mixer output on chip; call "
                                     "fmrx_pipeline_set_keep_intermediates(pl, 1) before processing");
        break;
    case FMRX_TAP_STEREO_FINAL: if (st) { src = pl->st_final.p; cnt = n_au; } break;
    default: return fail(FMRX_EINVAL, "read_tap: unknown tap %d", which);
    }
    if (which >= FMRX_TAP_CARRIER && !st) return fail(FMRX_EINVAL, "read_tap: tap %d exists only in stereo pipelines", which);
    *n = cnt;
    if (!out || cnt == 0) return FMRX_OK;
    if (which == FMRX_TAP_DEMOD && !pl->demod_valid)
        return fail(FMRX_EINVAL, "read_tap: the fused mono kernel keeps the discriminator output on chip; "
                                 "call fmrx_pipeline_set_keep_intermediates(pl, 1) before processing");
    if ((which == FMRX_TAP_IF_I || which == FMRX_TAP_IF_Q) && !pl->if_valid)
        return fail(FMRX_EINVAL, "read_tap: the IF stream is not materialised by the fused front end; call "
                                 "fmrx_pipeline_set_keep_intermediates(pl, 1) before processing");
    if (which == FMRX_TAP_IF_I || which == FMRX_TAP_IF_Q) {
        std::vector<float> z(2 * cnt);
        FMRX_HIP(hipMemcpy(z.data(), pl->ifb.p, 2 * cnt * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < cnt; k++) out[k] = z[2 * k + (which == FMRX_TAP_IF_Q)];
        return FMRX_OK;
    }
    FMRX_HIP(hipMemcpy(out, src, cnt * sizeof(float), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

// ---- carried state -----------------------------------------------------------------------
size_t fmrx_pipeline_state_size(const fmrx_pipeline *pl)
{
    if (!pl) return 0;
    size_t n = 2 * (pl->p.rf_taps - 1) + 2 + pl->Ha;
    if (pl->channels == 2) n += 2 * (pl->St - 1) + pl->Ha + pl->delay + 6;
    if (pl->de.on) n += 2 * pl->channels;   // de-emphasis: x_prev, y_prev per audio channel
    return n;
}

int fmrx_pipeline_get_state(fmrx_pipeline *pl, float *state, size_t n)
{
    if (!pl || !state) return fail(FMRX_EINVAL, "get_state: null argument");
    if (n != fmrx_pipeline_state_size(pl)) return fail(FMRX_EINVAL, "get_state: expected %zu floats", fmrx_pipeline_state_size(pl));
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_HIP(hipDeviceSynchronize());
    const int T = pl->p.rf_taps, hb = pl->fe.hist_bytes, live = 2 * (T - 1);
    std::vector<uint8_t> hist(hb);
    FMRX_HIP(hipMemcpy(hist.data(), pl->fe_hist[pl->fe_cur].p, hb, hipMemcpyDeviceToHost));
    float *o = state;
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < T - 1; i++) *o++ = (static_cast<int>(hist[hb - live + 2 * i + c]) - 128) / 128.0f;
    FMRX_HIP(hipMemcpy(o, pl->prev_iq[pl->prev_cur].p, 2 * sizeof(float), hipMemcpyDeviceToHost));
    o += 2;
    std::vector<float> dh(pl->Hd);
    // the carried demod history = the last Hd samples of [front | block] of the buffer used last
    FMRX_HIP(hipMemcpy(dh.data(), pl->demod_buf[pl->demod_last].p + pl->demod_n_last, pl->Hd * sizeof(float),
                       hipMemcpyDeviceToHost));
    // the demod history is shared by every consumer of demod; each reference
    // state vector is a window of it
    const float *dend = dh.data() + pl->Hd;  // one past demod[-1]
    // state_mono: audio FIR input is the all-passed demod: samples demod[-delay-Ha .. -delay-1]
    std::memcpy(o, dend - pl->delay - pl->Ha, pl->Ha * sizeof(float));
    o += pl->Ha;
    if (pl->channels == 2) {
        std::memcpy(o, dend - (pl->St - 1), (pl->St - 1) * sizeof(float)); o += pl->St - 1;  // state_stereo
        std::memcpy(o, dend - (pl->St - 1), (pl->St - 1) * sizeof(float)); o += pl->St - 1;  // state_carrier
        FMRX_HIP(hipMemcpy(o, pl->mix_tail[pl->mix_cur].p + (pl->Hm - pl->Ha), pl->Ha * sizeof(float), hipMemcpyDeviceToHost)); o += pl->Ha;  // state_stereofilt
        std::memcpy(o, dend - pl->delay, pl->delay * sizeof(float)); o += pl->delay;        // state_allpass
        FMRX_HIP(hipMemcpy(o, pl->pll_state.p, 6 * sizeof(float), hipMemcpyDeviceToHost)); o += 6;
    }
    if (pl->de.on) FMRX_HIP(hipMemcpy(o, pl->de.state.p, 2 * pl->channels * sizeof(float), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

int fmrx_pipeline_set_state(fmrx_pipeline *pl, const float *state, size_t n)
{
    if (!pl || !state) return fail(FMRX_EINVAL, "set_state: null argument");
    if (n != fmrx_pipeline_state_size(pl)) return fail(FMRX_EINVAL, "set_state: expected %zu floats", fmrx_pipeline_state_size(pl));
    FMRX_HIP(hipSetDevice(pl->device));
    FMRX_HIP(hipDeviceSynchronize());
    const int T = pl->p.rf_taps, hb = pl->fe.hist_bytes, live = 2 * (T - 1);
    std::vector<uint8_t> hist(hb, 128);
    const float *o = state;
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < T - 1; i++) {
            const float v = *o++ * 128.0f + 128.0f;
            if (!(v >= 0.0f && v <= 255.0f) || v != static_cast<float>(static_cast<int>(v)))
                return fail(FMRX_EINVAL, "set_state: front-end state holds a value that is not (u8-128)/128");
            hist[hb - live + 2 * i + c] = static_cast<uint8_t>(v);
        }
    const float *s_prev = o; o += 2;
    std::vector<float> dh(pl->Hd, 0.0f);
    float *dend = dh.data() + pl->Hd;
    const float *s_mono = o; o += pl->Ha;
    if (pl->channels == 2) {
        const float *s_st = o; o += pl->St - 1;
        const float *s_car = o; o += pl->St - 1;
        const float *s_sf = o; o += pl->Ha;
        const float *s_ap = o; o += pl->delay;
        // widest window first, then the ones that must agree with it
        std::memcpy(dend - pl->delay - pl->Ha, s_mono, pl->Ha * sizeof(float));
        std::memcpy(dend - pl->delay, s_ap, pl->delay * sizeof(float));
        std::memcpy(dend - (pl->St - 1), s_st, (pl->St - 1) * sizeof(float));
        // every consumer of the discriminator output reads ONE history here, of which the reference's vectors are windows
        // (state_carrier and state_stereo the same one): a state whose windows disagree is not a state of this receiver
        const int St1 = pl->St - 1;
        const int wm = St1 - pl->delay < pl->Ha ? St1 - pl->delay : pl->Ha;   // state_mono's samples inside state_stereo's window
        // (checked before anything is written: a refused state leaves the handle as it was)
        if (std::memcmp(s_car, s_st, St1 * sizeof(float)) != 0 ||
            std::memcmp(s_ap, s_st + St1 - pl->delay, pl->delay * sizeof(float)) != 0 ||
            std::memcmp(s_mono + pl->Ha - wm, s_st + St1 - pl->delay - wm, wm * sizeof(float)) != 0)
            return fail(FMRX_EINVAL, "set_state: state_stereo, state_carrier, state_allpass and state_mono are windows of one "
                                     "discriminator history and must agree where they overlap");
        FMRX_HIP(hipMemset(pl->mix_tail[pl->mix_cur].p, 0, pl->Hm * sizeof(float)));
        FMRX_HIP(hipMemcpy(pl->mix_tail[pl->mix_cur].p + (pl->Hm - pl->Ha), s_sf, pl->Ha * sizeof(float), hipMemcpyHostToDevice));
        FMRX_HIP(hipMemcpy(pl->pll_state.p, o, 6 * sizeof(float), hipMemcpyHostToDevice));
        pl->pll_off = static_cast<double>(o[5]);                   // trigOffset (src/filter.cpp:37)
        o += 6;
    } else {
        std::memcpy(dend - pl->Ha, s_mono, pl->Ha * sizeof(float));
    }
    FMRX_HIP(hipMemcpy(pl->fe_hist[pl->fe_cur].p, hist.data(), hb, hipMemcpyHostToDevice));
    FMRX_HIP(hipMemcpy(pl->prev_iq[pl->prev_cur].p, s_prev, 2 * sizeof(float), hipMemcpyHostToDevice));
    FMRX_HIP(hipMemcpy(pl->demod_buf[0].p, dh.data(), pl->Hd * sizeof(float), hipMemcpyHostToDevice));
    pl->demod_last = 0;
    pl->demod_n_last = 0;
    pl->demod_front[0] = true;
    pl->prev_override = true;   // the fused front end would otherwise recompute IF[-1] from the byte history
    pl->pll_warm = false;
    if (pl->channels == 2) FMRX_HIP(hipMemset(pl->pll_scratch.p + 5, 0, 3 * sizeof(float)));
    if (pl->de.on) FMRX_HIP(hipMemcpy(pl->de.state.p, o, 2 * pl->channels * sizeof(float), hipMemcpyHostToDevice));
    return FMRX_OK;
}

int fmrx_pipeline_last_timing(fmrx_pipeline *pl, float *t)
{
    int count = 0;
    FMRX_TRY(fmrx_pipeline_timing_sum(pl, t, &count, 1));
    return FMRX_OK;
}

int fmrx_pipeline_timing_sum(fmrx_pipeline *pl, float *t, int *count, int max_calls)
{
    if (!pl || !t || !count) return fail(FMRX_EINVAL, "timing_sum: null argument");
    if (pl->calls == 0) return fail(FMRX_EINVAL, "timing: no profiled process call (enable with fmrx_pipeline_set_profiling)");
    unsigned long n = pl->calls < static_cast<unsigned long>(fmrx_pipeline::kRing) ? pl->calls : fmrx_pipeline::kRing;
    if (max_calls > 0 && static_cast<unsigned long>(max_calls) < n) n = max_calls;
    t[0] = t[1] = t[2] = t[3] = 0.0f;
    for (unsigned long i = 0; i < n; i++) {
        hipEvent_t *ev = pl->ev[(pl->calls - 1 - i) % fmrx_pipeline::kRing];
        FMRX_HIP(hipEventSynchronize(ev[3]));
        float d[4];
        FMRX_HIP(hipEventElapsedTime(&d[0], ev[0], ev[1]));
        FMRX_HIP(hipEventElapsedTime(&d[1], ev[1], ev[2]));
        FMRX_HIP(hipEventElapsedTime(&d[2], ev[2], ev[3]));
        FMRX_HIP(hipEventElapsedTime(&d[3], ev[0], ev[3]));
        for (int k = 0; k < 4; k++) t[k] += d[k];
    }
    *count = static_cast<int>(n);
    return FMRX_OK;
}

}  // extern "C"
