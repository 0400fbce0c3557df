// bank.hip -- a bank of N independent receivers per device call, host side (include/fmrx.h: fmrx_channels_create_ex): the handle's
// buffers, the two-stream chunk schedule of a stereo call, reset and tap read-back, for every kind of bank.  The kernels, their
// tables and launchers are kernels_bank.hip's, which also says what the banks with rows compute and how the rows are laid out; the
// fast mono bank of modes 0/1 keeps no rows (below: plan_fused) and runs the fused mono kernel of kernels_fe_mfma.hip.
#include "bank_kernels.hpp"

namespace fmrx {

Bank::~Bank()
{
    for (hipStream_t st : {wide, lanes, front})
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    for (auto *evs : {ev_bpf, ev_pll, ev_fe})
        for (int i = 0; i < kMaxChunks; i++)
            if (evs[i]) (void)hipEventDestroy(evs[i]);
    for (hipEvent_t e : {ev_fork, ev_join})
        if (e) (void)hipEventDestroy(e);
}

namespace {

template <typename T>
int zeroed(DevBuf<T> &d, size_t count)
{
    FMRX_TRY(d.alloc(count));
    FMRX_HIP(hipMemset(d.p, 0, d.bytes()));
    return FMRX_OK;
}

// IF samples [.., if_of(a)) are what the audio outputs [.., a) read: a * D in the integer-decimation modes, whole periods
// (U outputs <-> D samples) in the resampling modes
long if_of(const Bank &b, long a) { return b.resample ? a / b.p.audio_upsamp * b.p.audio_decim : a * b.p.audio_decim; }

void plan_chunks(Bank &b)
{
    // chunks of whole output workgroups (512 audio samples; whole periods of U outputs in the resampling modes);
    // chunk c = audio [a_c, a_c+1) = IF [if_of(a_c), if_of(a_c+1))
    const long unit = b.resample ? b.p.audio_upsamp : 512;
    b.per = (b.n_audio + Bank::kMaxChunks - 1) / Bank::kMaxChunks;
    b.per = (b.per + unit - 1) / unit * unit;
    b.K = static_cast<int>((b.n_audio + b.per - 1) / b.per);
    // fast banks: the front end is HBM-bound on the matrix cores, the band-pass pair and the output stage are bound by the
    // vector ALUs: on two streams they run side by side
    b.split = b.K > 1 && !b.exact;
    // The output stage of chunk c follows the band-pass pair of chunk c + lag on the wide stream.  Exact banks: lag 1 (the PLL is
    // the longest stage; nothing on the wide stream is waited for).  Fast banks: lag 2 -- the PLL of chunk c starts when its
    // band-pass pair ends and takes longer than the next chunk's band-pass pair: with lag 1 the wide stream idled a third
    // of the time waiting for it.
    b.lag = (b.exact || b.K < 3) ? 1 : 2;
    // the front end works in whole tiles of its own (63 x 8 outputs per wave; 120 per matrix-core tile): its share of a chunk
    // ends on the first tile boundary at or behind the chunk's end, so that no chunk pays for a partly filled last tile
    // (2560-sample chunks are 5.08 tiles of 504: 15 % of the exact front end's work was computed and thrown away)
    b.fe_tile = b.exact ? 63 * kR : 120;
    // fast banks, modes 0/1: the cosine is taken inside the output stage; the resampling modes materialise the mixer rows from
    // finished NCO values
    b.nco_pass = b.exact || b.resample;
}

// the pilot PLL over IF samples [k_lo, k_hi) of every channel, lane = channel: exact banks read the pilot band-pass row, fast
// banks its sign row; the first chunk of a call also leaves PLL[0] in nco0
int launch_pll(const Bank &b, long k_lo, long k_hi, bool first, hipStream_t s)
{
    const float *in = b.exact ? b.carrier.p + k_lo : reinterpret_cast<const float *>(b.carrier8.p + k_lo);
    return k_fm_pll_channels(in, b.exact ? b.ypitch : b.cpitch, static_cast<size_t>(k_hi - k_lo), b.n_channels, b.trig.p + k_lo, b.ypitch,
                             b.pll.p, first ? b.nco0.p : nullptr, kPilotHz, static_cast<float>(b.p.if_Fs), kNcoScale, kPhaseAdjust,
                             kPllBandwidth, s, true, b.exact != 0, !b.exact);
}

int process_stereo(Bank *b, float *d_audio, int16_t *d_pcm, int wrap, hipStream_t s)
{
    const long K = b->K, lag = b->lag, per = b->per;
    hipStream_t sw = K > 1 ? b->wide : s, sl = K > 1 ? b->lanes : s;
    hipStream_t sf = b->split ? b->front : sw;
    if (K > 1) {   // whatever the caller's stream did before the call (loading the slots, reading the last output) comes first
        FMRX_HIP(hipEventRecord(b->ev_fork, s));
        FMRX_HIP(hipStreamWaitEvent(sw, b->ev_fork, 0));
        FMRX_HIP(hipStreamWaitEvent(sl, b->ev_fork, 0));
        if (b->split) FMRX_HIP(hipStreamWaitEvent(sf, b->ev_fork, 0));
    }
    long fe_done = 0;
    for (int c = 0; c < K + lag; c++) {
        if (c < K) {
            const long a_lo = c * per, a_hi = a_lo + per < b->n_audio ? a_lo + per : b->n_audio;
            const long k_lo = if_of(*b, a_lo), k_hi = if_of(*b, a_hi);
            long fe_hi = (k_hi + b->fe_tile - 1) / b->fe_tile * b->fe_tile;
            if (fe_hi > b->n_if || c == K - 1) fe_hi = b->n_if;
            if (fe_hi > fe_done) FMRX_TRY(b->k.fe(*b, fe_done, fe_hi, sf));
            fe_done = fe_hi;
            if (b->split) {   // read-after-write: the band-pass pair reads the discriminator rows the front end wrote on its own stream
                FMRX_HIP(hipEventRecord(b->ev_fe[c], sf));
                FMRX_HIP(hipStreamWaitEvent(sw, b->ev_fe[c], 0));
            }
            FMRX_TRY(b->k.bpf(*b, k_lo, k_hi, sw));
            if (K > 1) {
                FMRX_HIP(hipEventRecord(b->ev_bpf[c], sw));
                FMRX_HIP(hipStreamWaitEvent(sl, b->ev_bpf[c], 0));
            }
            FMRX_TRY(launch_pll(*b, k_lo, k_hi, c == 0, sl));
            if (K > 1) FMRX_HIP(hipEventRecord(b->ev_pll[c], sl));
        }
        if (c >= lag) {   // the output stage of an earlier chunk, behind this chunk's band-pass pair on the wide stream
            const long a_lo = (c - lag) * per, a_hi = a_lo + per < b->n_audio ? a_lo + per : b->n_audio;
            if (K > 1) FMRX_HIP(hipStreamWaitEvent(sw, b->ev_pll[c - lag], 0));   // (the PLL followed this chunk's band-pass pair: both are done)
            if (b->nco_pass)
                FMRX_TRY(bank_launch_nco(b->exact, b->trig.p, b->ypitch, b->n_channels, if_of(*b, a_lo), if_of(*b, a_hi), b->bpf.p, b->nco0.p,
                                         b->resample ? b->mixer.p : nullptr, b->mpitch, b->Hm, sw));
            FMRX_TRY(b->k.out(*b, d_audio, d_pcm, wrap, a_lo, a_hi, if_of(*b, a_hi), sw));
        }
    }
    if (K > 1) {
        FMRX_HIP(hipEventRecord(b->ev_join, sw));               // the last output stage follows everything else of the call
        FMRX_HIP(hipStreamWaitEvent(s, b->ev_join, 0));
    }
    b->mix_cur ^= 1;
    return FMRX_OK;
}

int process_mono(Bank *b, float *d_audio, int16_t *d_pcm, int wrap, hipStream_t s)
{
    FMRX_TRY(b->k.fe(*b, 0, b->n_if, s));
    return b->k.out(*b, d_audio, d_pcm, wrap, 0, b->n_audio, b->n_if, s);
}

// the slots of all channels as one pseudo-stream that starts in silence; the audio / PCM of whole slots, for the finish kernel to compact
int process_fused(Bank *b, float *d_audio, int wrap, hipStream_t s)
{
    const float *zend = b->zeros.p + b->p.audio_taps + 32;     // "one past the previous block's last discriminator sample": zeros
    return mono_fused_launch(b->fe, b->audio, b->slots.p, b->slot_bytes * b->n_channels / 2, b->fe.silence.p, b->zeros.p, zend, nullptr, 0,
                             nullptr, d_audio ? b->audio_all.p : nullptr, b->pcm_all.p, wrap, nullptr, b->opt, s);
}

// The fused kind (mono, fast, modes 0/1).  The mono chain of modes 0/1 is a sliding-window map of its input
// (SURVEY A.4): audio sample k depends on the rf_decim*(audio_taps) + rf_taps - 1 complex input samples in front of it (1 110 at
// 101/101 taps) and on nothing else, so a channel's whole carried state (I/Q FIR state, prev_i/prev_q, state_mono) is its last
// 1 110 input samples: the history in front of its slot.  Audio samples whose window reaches back into the previous slot (the
// first junk_audio of every slot: 28 at 101/101 taps, 2.3 % extra work at the reference's block size) are computed and thrown
// away; all others see exactly the samples the streaming pipeline would have seen: IF and discriminator values bit-identical to
// fmrx_pipeline's, audio equal to within the float32 summation order of the fused kernel's MFMA tiles (<= 2e-6).
int plan_fused(Bank &b, const Filters &f)
{
    const fmrx_params &p = b.p;
    FMRX_TRY(fe_plan_init(b.fe, f.rf.data(), p.rf_taps, p.rf_decim));
    FMRX_TRY(audio_plan_init(b.audio, f.audio.data(), p.audio_taps, p.audio_decim));
    // samples an audio output reaches back: rf_decim*audio_taps + rf_taps - 1, plus what the kernel's tiles read in
    // front of a run (one IF sample for the discriminator, 16-byte rounding): rounded up to whole audio samples
    // and 16-byte multiples
    const size_t unit = static_cast<size_t>(2) * p.rf_decim * p.audio_decim;   // bytes per audio sample
    const size_t reach = static_cast<size_t>(p.rf_decim) * (p.audio_taps + 1) + p.rf_taps + 8 * p.rf_decim;
    size_t hs = (reach * 2 + unit - 1) / unit * unit;
    while (hs % 16) hs += unit;
    b.hist_bytes = hs;
    b.junk_audio = hs / unit;
    return FMRX_OK;
}

// Every other kind: the tables of its stages, and the histories in front of a channel's slot and rows.
int plan_rows(Bank &b, const Filters &f)
{
    const fmrx_params &p = b.p;
    const bool stereo = b.audio_channels == 2;
    FMRX_TRY(b.k.fe_table(b, f.rf.data()));
    b.hist_bytes = b.k.hist_bytes;
    if (!b.exact) {   // the matrix-core front end (int8 MFMA on the raw bytes): its tap image, and the history its windows reach
        FMRX_TRY(fe_plan_init(b.fe, f.rf.data(), p.rf_taps, p.rf_decim));
        const int lead = fe_mfma_bank_lead(b.fe);
        if (!b.fe.mfma || lead < 0) return fail(FMRX_EINVAL, "channels: no matrix-core front end for rf %d taps / decim %d", p.rf_taps, p.rf_decim);
        const size_t need = (static_cast<size_t>(lead) + 15) / 16 * 16;
        if (need > b.hist_bytes) b.hist_bytes = need;
    }
    FMRX_TRY(b.k.out_table(b, f.audio.data()));
    b.Ha = b.resample ? (p.audio_taps - 1) / p.audio_upsamp : p.audio_taps - 1;
    b.delay = stereo ? (p.stereo_taps - 1) / 2 : 0;                        // allPass, src/filter.cpp:14-29
    b.Hd = b.Ha + b.delay;
    if (stereo && p.stereo_taps - 1 + 3 > b.Hd) b.Hd = p.stereo_taps - 1 + 3;
    const int more = b.res_hist > b.Ha ? b.res_hist - b.Ha : 0;   // (the lane-per-channel resampler rounds its windows up to whole iterations)
    if (b.Ha + b.delay + more > b.Hd) b.Hd = b.Ha + b.delay + more;
    b.Hd = (b.Hd + 3) / 4 * 4 + 4;
    b.Hm = (b.Ha + more + 3) / 4 * 4 + 4;
    b.dpitch = (b.Hd + b.n_if + 16 + 3) / 4 * 4;
    b.ypitch = (b.n_if + 16 + 3) / 4 * 4;
    plan_chunks(b);
    return FMRX_OK;
}

}  // namespace

int bank_create(std::unique_ptr<Bank> &out, const fmrx_params &p, int n_channels, int audio_channels, int exact, size_t block_bytes,
                const Options &opt)
{
    const bool stereo = audio_channels == 2;
    if (p.audio_upsamp > 0 && p.audio_taps % p.audio_upsamp != 0)   // as fmrx_pipeline_create: the reference is a stream only then
        return fail(FMRX_EINVAL, "channels: audio_taps %d is not a multiple of audio_upsamp %d", p.audio_taps, p.audio_upsamp);
    std::unique_ptr<Bank> b(new Bank);   // (a failure below frees what was built so far)
    if (!bank_resolve(p, audio_channels, exact, b->k))
        return fail(FMRX_EINVAL, "channels (exact): no reference-order kernels for rf %d/%d, audio %d/%d, stereo %d taps (modes 0 and 1 of the "
                    "reference's tap sets are covered)", p.rf_taps, p.rf_decim, p.audio_taps, p.audio_decim, p.stereo_taps);
    const bool fused = b->k.fused;
    b->p = p;
    b->n_channels = n_channels;
    b->audio_channels = audio_channels;
    b->exact = exact ? 1 : 0;
    b->opt = opt;
    b->resample = p.audio_upsamp > 0;
    b->n_if = static_cast<long>(block_bytes / 2) / p.rf_decim;
    b->n_audio = b->resample ? b->n_if * p.audio_upsamp / p.audio_decim : b->n_if / p.audio_decim;
    const Filters f = design_filters(p, stereo);
    FMRX_TRY(fused ? plan_fused(*b, f) : plan_rows(*b, f));
    if (b->resample && (b->n_if * p.audio_upsamp) % p.audio_decim)
        return fail(FMRX_EINVAL, "channels: n_if * upsamp = %ld is not a multiple of audio_decim %d (a block must end on an output boundary)",
                    b->n_if * p.audio_upsamp, p.audio_decim);
    // (the finish kernels copy the tail of a slot and of a row to its front: the two must not overlap)
    if (block_bytes < b->hist_bytes || b->n_if < b->Hd)
        return fused ? fail(FMRX_EINVAL, "channels_create: block_bytes %zu < the %zu bytes of history a channel carries", block_bytes, b->hist_bytes)
                     : fail(FMRX_EINVAL, "channels (exact): block of %zu bytes is shorter than the history a channel carries (%zu bytes, %d IF samples)",
                            block_bytes, b->hist_bytes, b->Hd);
    b->slot_bytes = b->hist_bytes + block_bytes;
    const size_t N = static_cast<size_t>(n_channels), total = b->slot_bytes * N;
    if (fused && !mono_fused_available(b->fe, b->audio, reinterpret_cast<const uint8_t *>(16), total / 2, reinterpret_cast<const uint8_t *>(16)))
        return fail(FMRX_EINVAL, "channels_create: no fused mono kernel for rf_taps %d / decim %d / audio_taps %d / decim %d",
                    p.rf_taps, p.rf_decim, p.audio_taps, p.audio_decim);
    // the kernels' last loads run on behind the last slot (results discarded): the exact front end's last tile by 63*R outputs' worth of bytes
    FMRX_TRY(b->slots.alloc(total + 64 + (fused ? 0 : 2 * 64 * kR * p.rf_decim)));
    FMRX_TRY(k_fill_u8(b->slots.p, b->slots.n, 128, nullptr));                            // silence: a stream that starts here
    if (fused) {
        FMRX_TRY(zeroed(b->zeros, p.audio_taps + 64));
        const size_t all = N * (b->junk_audio + b->n_audio);   // the audio of whole slots, junk included
        FMRX_TRY(b->audio_all.alloc(all + 16));
        FMRX_TRY(b->pcm_all.alloc(all + 16));
    } else {
        FMRX_TRY(zeroed(b->demod, b->dpitch * N + 64));
    }
    if (stereo) {
        FMRX_TRY(b->k.bpf_table(*b, f.stereo.data(), f.pilot.data()));
        if (b->exact) {
            FMRX_TRY(zeroed(b->carrier, b->ypitch * N + 64));
        } else {
            b->cpitch = (b->n_if + 64 + 15) / 16 * 16;
            FMRX_TRY(zeroed(b->carrier8, b->cpitch * N + 64));
        }
        FMRX_TRY(b->bpf.alloc(b->ypitch * N + 64));
        FMRX_TRY(b->trig.alloc(b->ypitch * N + 64));
        FMRX_TRY(b->pll.alloc(8 * N));
        FMRX_TRY(b->nco0.alloc(N));
        for (auto &m : b->mixtail) FMRX_TRY(zeroed(m, static_cast<size_t>(b->Hm) * N));
        if (b->resample) {
            b->mpitch = (b->Hm + b->n_if + 16 + 3) / 4 * 4;
            FMRX_TRY(zeroed(b->mixer, b->mpitch * N + 64));
        }
        FMRX_TRY(bank_launch_fill_state(b->pll.p, static_cast<long>(8 * N), nullptr));
        for (hipStream_t *st : {&b->wide, &b->lanes, &b->front}) FMRX_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
        for (auto *evs : {b->ev_fe, b->ev_bpf, b->ev_pll})
            for (int i = 0; i < Bank::kMaxChunks; i++) FMRX_HIP(hipEventCreateWithFlags(&evs[i], hipEventDisableTiming));
        for (hipEvent_t *e : {&b->ev_fork, &b->ev_join}) FMRX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    FMRX_HIP(hipDeviceSynchronize());
    out = std::move(b);
    return FMRX_OK;
}

size_t bank_n_audio(const Bank *b) { return static_cast<size_t>(b->n_audio); }
void bank_input_layout(const Bank *b, uint8_t **d_first_block, size_t *pitch_bytes)
{
    *d_first_block = b->slots.p + b->hist_bytes;
    *pitch_bytes = b->slot_bytes;
}
int bank_demod_layout(const Bank *b, const float **d_row0, size_t *pitch, size_t *n_if)
{
    if (b->k.fused) return fail(FMRX_EINVAL, "channels_demod_layout: the fused mono bank of modes 0/1 keeps no discriminator rows");
    *d_row0 = b->demod.p + b->Hd;   // the finish kernel rewrites only the history in front of each row
    *pitch = static_cast<size_t>(b->dpitch);
    *n_if = static_cast<size_t>(b->n_if);
    return FMRX_OK;
}

// back to the start-of-stream state (src/project.cpp:61-65, 446-458): one channel, or all of them (channel < 0).  One channel:
// the history in front of its slot and of each of its rows; the whole bank: the same buffers whole, one fill each.
int bank_reset(Bank *b, int channel)
{
    FMRX_HIP(hipDeviceSynchronize());
    const bool all = channel < 0;
    const size_t c = all ? 0 : channel, nc = all ? b->n_channels : 1;
    auto zero = [&](DevBuf<float> &buf, long pitch, int hist) {
        if (!buf.p) return hipSuccess;   // rows this bank does not keep
        return all ? hipMemsetAsync(buf.p, 0, buf.bytes(), nullptr) : hipMemsetAsync(buf.p + c * pitch, 0, hist * sizeof(float), nullptr);
    };
    FMRX_TRY(k_fill_u8(b->slots.p + c * b->slot_bytes, all ? b->slot_bytes * nc : b->hist_bytes, 128, nullptr));
    FMRX_HIP(zero(b->demod, b->dpitch, b->Hd));
    if (b->audio_channels == 2) {
        for (auto &m : b->mixtail) FMRX_HIP(zero(m, b->Hm, b->Hm));
        if (b->resample) FMRX_HIP(zero(b->mixer, b->mpitch, b->Hm));
        FMRX_TRY(bank_launch_fill_state(b->pll.p + 8 * c, static_cast<long>(8 * nc), nullptr));
    }
    FMRX_HIP(hipDeviceSynchronize());
    return FMRX_OK;
}

// d_audio: [n_channels][audio_channels][n_audio] (stereo: left, then right); d_pcm: [n_channels][n_audio][audio_channels]
int bank_process_dev(Bank *b, float *d_audio, int16_t *d_pcm, int wrap, hipStream_t s)
{
    FMRX_TRY(b->k.fused ? process_fused(b, d_audio, wrap, s)
                        : b->audio_channels == 2 ? process_stereo(b, d_audio, d_pcm, wrap, s) : process_mono(b, d_audio, d_pcm, wrap, s));
    return bank_launch_finish(*b, d_audio, d_pcm, s);
}

// diagnostics / tests: one channel's row of an intermediate of the last call.  which: FMRX_TAP_DEMOD, _CARRIER (fast banks: the
// sign row the PLL reads, as -1 / 0 / +1), _STEREO_BPF, _PLL (n_if + 1 values: PLL[0] = the state's lastOut, then the finished
// NCO values), _TRIG_ARG (fast banks of modes 0/1: the raw trigArg of every step -- their output stage takes the cosine on chip,
// the row stays raw; the other banks' NCO pass overwrites it in place)
int bank_read_tap(Bank *b, int channel, int which, float *out, size_t *n)
{
    if (b->k.fused)
        return fail(FMRX_EINVAL, "channels_read_tap: the fused mono bank of modes 0/1 keeps no intermediates in memory (stereo, exact and "
                    "resampling-mode banks do)");
    if (channel < 0 || channel >= b->n_channels) return fail(FMRX_EINVAL, "channels_read_tap: channel %d of %d", channel, b->n_channels);
    FMRX_HIP(hipDeviceSynchronize());
    const size_t n_if = static_cast<size_t>(b->n_if);
    const bool stereo = b->audio_channels == 2;
    const float *src = nullptr;
    size_t cnt = n_if;
    switch (which) {
    // the finish kernel has copied the row's tail into its front already; the block itself is intact
    case FMRX_TAP_DEMOD: src = b->demod.p + channel * b->dpitch + b->Hd; break;
    case FMRX_TAP_CARRIER:
        if (stereo && !b->exact) {
            *n = cnt;
            if (!out) return FMRX_OK;
            std::vector<int8_t> sg(n_if);
            FMRX_HIP(hipMemcpy(sg.data(), b->carrier8.p + channel * b->cpitch, n_if, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < n_if; k++) out[k] = static_cast<float>(sg[k]);
            return FMRX_OK;
        }
        if (stereo) src = b->carrier.p + channel * b->ypitch;
        break;
    case FMRX_TAP_STEREO_BPF: if (stereo) src = b->bpf.p + channel * b->ypitch; break;
    case FMRX_TAP_PLL: if (stereo) { src = b->trig.p + channel * b->ypitch; cnt = n_if + 1; } break;
    case FMRX_TAP_TRIG_ARG: if (stereo && !b->nco_pass) src = b->trig.p + channel * b->ypitch; break;
    default: break;
    }
    if (!src) return fail(FMRX_EINVAL, "channels_read_tap: tap %d is not kept by this bank", which);
    *n = cnt;
    if (!out) return FMRX_OK;
    if (which == FMRX_TAP_PLL) {
        FMRX_HIP(hipMemcpy(out, b->nco0.p + channel, sizeof(float), hipMemcpyDeviceToHost));
        out++;
        cnt = n_if;
        if (!b->nco_pass) {
            // the fast bank of modes 0/1 keeps the raw trigArg of every step (the cosine is taken inside the output stage): the same
            // NCO pass the other banks run, here on a copy of the one row
            DevBuf<float> tmp;
            FMRX_TRY(tmp.alloc(static_cast<size_t>(b->ypitch)));
            FMRX_HIP(hipMemcpy(tmp.p, src, n_if * sizeof(float), hipMemcpyDeviceToDevice));
            FMRX_TRY(bank_launch_nco(false, tmp.p, b->ypitch, 1, 0, b->n_if, nullptr, nullptr, nullptr, 0, 0, nullptr));
            FMRX_HIP(hipMemcpy(out, tmp.p, n_if * sizeof(float), hipMemcpyDeviceToHost));
            return FMRX_OK;
        }
    }
    FMRX_HIP(hipMemcpy(out, src, cnt * sizeof(float), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

}  // namespace fmrx
