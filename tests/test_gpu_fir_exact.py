"""The packed-FMA FIR kernels checked BIT FOR BIT against the fma-chain model of tests/_fir_model.py, given the input
taps the kernels read:

  bpf_pair_kernel (kernels_stereo.hip)          carrier_filt, stereo_filt = the DESCENDING chain of the demod stream
  stereo_out_kernel (kernels_stereo.hip)        mixer = (stereo_filt * PLL) * 2; mono_filt, stereo_final = the ascending
                                                chain (mono `delay` samples back); L = st + mono, R = mono - st; PCM
  audio_fir_kernel (kernels_audio.hip)          mono audio of modes 0/1 (two-kernel path) = the polyphase chain
  chs_bpf_kernel, chs_out_kernel (kernels_bank.hip, fast bank)      stereo_filt, L/R = the ascending chain; the bank's
                                                IF equals the single-stream pipeline's bit for bit
  chs_resample_lanes_kernel (fast bank, 2/3)    L/R = the reference's resampler order with one fma per tap, on the delayed
                                                demod and the mixer

Each model is fed the stream the kernel read: the tap concatenated over the calls, zeros before the stream's start.  So a
wrong history sample at a block, chunk or workgroup seam, a wrong PLL[0], a tap out of place or a stale buffer read across
internal streams changes bits here, where an RMS tolerance would not see it (the Hann-windowed taps make h[0] exactly 0
and h[T-1] about 5e-5 of the peak).  Every synthetic-signal block with >= 1000 outputs also has to differ from the
reference-order result (ref_chain): the specialised kernel ran, not the generic fallback.

Inputs: the synthetic FM streams of tests/test_gpu_channels.py, and a stream of byte-128 silence (outputs exact zeros)
followed by full-scale 0/255 bytes.  Blocks: the reference's, n_if not a multiple of 8 (the tail path of the band-pass
kernels), the shortest the pipeline accepts (below the mixer history Hm where the tap counts allow it: stereo_out's
short-block tail), blocks spanning several workgroups, ~1 024 000-sample blocks, and one block of more tiles than
audio_fir_kernel has persistent workgroups (each of those walks two tiles).

The f32 matrix-core sums (the audio FIR inside mono_fused_kernel, resample_mfma_kernel) are pinned the same way, bit for
bit against an fmaf-chain model, by tests/test_gpu_mfma_exact.py; the two fast MONO banks -- the fused mono bank of modes
0/1 (mono_fused_kernel over all slots, at each channel's row phase, with channels_finish_kernel) and
chs_resample_lanes_kernel<STEREO = false> of modes 2/3 -- by tests/test_gpu_mono_banks_exact.py, which also runs the lane
resampler, mono and stereo, with more than one group per wave.

Out of scope, on purpose:
  * the PLL and the discriminator's v_rcp_f32 (the PLL's output is an input tap here, as the discriminator's is; the
    fast PLL is pinned against its own model by tests/test_gpu_pll_exact.py, the fast discriminator sample by sample
    against a model given the device's reciprocal by tests/test_gpu_demod_exact.py);
  * the exact banks: already bit for bit against the oracle (tests/test_gpu_channels.py);
  * the fast mono banks (tests/test_gpu_mono_banks_exact.py, above)."""
import math

import numpy as np
import pytest

import _fir_model as fm
from test_gpu_channels import channel_stream

pytestmark = pytest.mark.gpu

BPF_TAPS = [13, 101, 151]                              # FMRX_BPF_CASES
AUDIO_SHAPES = [(101, 5), (101, 6), (13, 5), (13, 6)]  # FMRX_AUDIO_CASES
STEREO_OUT_SHAPES = list(AUDIO_SHAPES)                 # stereo_out_launch's X(...) list
CHS_BPF_TAPS = [101, 151, 13]                          # CHS_BPF_CASES
CHS_OUT_SHAPES = list(AUDIO_SHAPES)                    # CHS_OUT_CASES
MODE_OF_DECIM = {5: 0, 6: 1}
# (mode, audio taps, stereo taps): every band-pass shape in every mode, every stereo_out shape in modes 0/1
STEREO_CASES = [(m, a, s) for m in (0, 1) for a in (101, 13) for s in BPF_TAPS] + [(m, 101, s) for m in (2, 3) for s in BPF_TAPS]
# (mode, (rf, audio, stereo) taps, receivers, reference blocks per call)
BANK_CONFIGS = [(0, (101, 101, 101), 24, 1), (0, (101, 101, 101), 65, 4), (1, (101, 101, 101), 24, 1), (1, (101, 101, 101), 65, 4),
                (0, (13, 13, 13), 24, 1), (1, (13, 13, 13), 24, 1), (0, (151, 101, 151), 65, 4)]
MIN_POWER = 1000     # outputs per block from which the fma chain must differ from the reference's order


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bits_equal(got, want, msg):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape, msg)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert len(bad) == 0, f"{msg}: {len(bad)} of {len(got)} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def differs(got, ref):
    return bool((bits(got) != bits(ref)).any())


def silence_then_full_scale(n_samples, silent, seed=7):
    """Byte 128 (0.0 after conversion) for `silent` complex samples, then random 0 / 255 bytes."""
    iq = np.full(2 * n_samples, 128, np.uint8)
    rng = np.random.default_rng(seed)
    iq[2 * silent:] = rng.integers(0, 2, 2 * (n_samples - silent)).astype(np.uint8) * 255
    return iq


def taps_of(fmrx, p):
    fs = float(p.if_Fs)
    au_fs = fs * p.audio_upsamp if p.audio_upsamp else fs
    return (fmrx.bandPass(fs, 22e3, 54e3, p.stereo_taps), fmrx.bandPass(fs, 18.5e3, 19.5e3, p.stereo_taps),
            fmrx.impulseResponseLPF(au_fs, 16e3, p.audio_taps))


def ref_n_if(p):
    return p.block_bytes // 2 // p.rf_decim


def block_cuts(p, stereo, big=False):
    """IF samples per block: reference, tail path, shortest accepted, several workgroups, reference (and ~1 024 000
    complex samples)."""
    D, ref = p.audio_decim, ref_n_if(p)
    if p.audio_upsamp:
        unit = D // math.gcd(D, p.audio_upsamp)
        return [ref, unit * math.ceil(max(ref // 7, p.stereo_taps) / unit), 2 * ref, ref]
    need = max(p.audio_taps - 1, p.stereo_taps - 1 if stereo else 0, -(-(p.rf_taps - 1) // p.rf_decim))
    short = D * math.ceil(need / D)
    cuts = [ref, ref + D, short, D * 2603, ref]
    assert (ref + D) % 8 and (D * 2603) % 8 and D * 2603 > 2 * 2048
    if big:
        cuts.append(D * math.ceil(1_024_000 // p.rf_decim / D))
    return cuts


def feed(cuts, p, iq):
    """The blocks of `iq` cut as `cuts` (IF samples each)."""
    out, o = [], 0
    for n_if in cuts:
        nb = 2 * n_if * p.rf_decim
        out.append(iq[o:o + nb])
        o += nb
    assert o <= len(iq)
    return out


def stream_bytes(cuts, p):
    return 2 * sum(cuts) * p.rf_decim


def concat(blocks, name):
    return np.concatenate([b[name] for b in blocks])


def offsets(blocks, name):
    o = np.cumsum([0] + [len(b[name]) for b in blocks])
    return list(zip(o[:-1], o[1:]))


def check_blocks(blocks, name, want, msg, ref=None, power_ok=None):
    for b, (lo, hi) in enumerate(offsets(blocks, name)):
        bits_equal(blocks[b][name], want[lo:hi], f"{msg}: {name}, block {b} ({hi - lo} samples)")
        if ref is not None and power_ok and hi - lo >= MIN_POWER:
            assert differs(blocks[b][name], ref[lo:hi]), f"{msg}: {name} block {b} equals the reference order (generic kernel?)"


def stereo_streams(oracle, p, cuts):
    n = stream_bytes(cuts, p) // 2
    return [("synthetic", channel_stream(oracle, 0, n, p.rf_Fs), True),
            ("silence + full scale", silence_then_full_scale(n, n // 3), False)]


# ---- a. single-stream stereo ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,audio_taps,stereo_taps", STEREO_CASES)
def test_single_stream_stereo(fmrx, oracle, mode, audio_taps, stereo_taps):
    """bpf_pair_kernel (every mode) and stereo_out_kernel (modes 0/1) against the model, intermediates kept."""
    p = fmrx.modeParams(mode, 101, audio_taps, stereo_taps)
    h_st, h_car, h_au = taps_of(fmrx, p)
    cuts = block_cuts(p, True)
    D, delay, fused = p.audio_decim, (p.stereo_taps - 1) // 2, mode in (0, 1)
    for label, iq, power in stereo_streams(oracle, p, cuts):
        pl = fmrx.Pipeline(mode, 2, params=p, max_block_bytes=2 * max(cuts) * p.rf_decim)
        pl.set_keep_intermediates(True)
        blocks = []
        for blk in feed(cuts, p, iq):
            out = pl.process(blk)
            r = {k: pl.read_tap(k) for k in ("demod", "carrier_filt", "stereo_filt", "pll")}
            if fused:
                r.update({k: pl.read_tap(k) for k in ("mixer", "mono_filt", "stereo_final")})
                r.update(audio_l=out["audio_l"], audio_r=out["audio_r"], pcm_l=out["pcm16"][0::2], pcm_r=out["pcm16"][1::2])
            blocks.append(r)
        pl.close()
        tag = f"mode {mode} taps {audio_taps}/{stereo_taps} {label}"
        x = concat(blocks, "demod")
        sf, car = fm.bpf_pair(x, h_st, h_car)
        check_blocks(blocks, "stereo_filt", sf, tag, fm.ref_chain(x, h_st), power)
        check_blocks(blocks, "carrier_filt", car, tag, fm.ref_chain(x, h_car), power)
        if not power:
            silent = len(iq) // 6 // p.rf_decim - p.rf_taps        # IF samples whose front-end window is all silence
            assert silent > 1000 and not x[:silent].any() and not sf[:silent].any() and not car[:silent].any()
        if not fused:
            continue
        for b in blocks:
            bits_equal(b["mixer"], fm.mixer(b["stereo_filt"], b["pll"]), tag + ": mixer tap")
        mono, st = fm.audio_pair(x, concat(blocks, "mixer"), h_au, D, delay, fm.ascending(p.audio_taps))
        check_blocks(blocks, "mono_filt", mono, tag, fm.ref_chain(x, h_au, D, delay), power)
        check_blocks(blocks, "stereo_final", st, tag)
        left, right = fm.combine(st, mono)
        check_blocks(blocks, "audio_l", left, tag)
        check_blocks(blocks, "audio_r", right, tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_l"), oracle.pcm16(left), tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_r"), oracle.pcm16(right), tag)
        if not power:
            assert not left[:silent // D - p.audio_taps].any() and not right[:silent // D - p.audio_taps].any()


@pytest.mark.parametrize("mode,lanes", [(0, 1), (1, 1), (0, 2), (1, 2)])
def test_stereo_lr_overlapped_calls(fmrx, oracle, mode, lanes):
    """L/R with intermediates off, plain and under option overlap_calls (front end | PLL | output stage of consecutive calls
    on internal streams, two buffer sets): the model's, fed the plain pipeline's demod, stereo_filt and pll taps.  The
    mixer comes from those taps; no read_tap here needs the materialised mixer."""
    import torch
    p = fmrx.modeParams(mode)
    calls, nb = 4, 2 * p.block_bytes
    iq = channel_stream(oracle, 5, calls * nb // 2, p.rf_Fs)
    h_st, h_car, h_au = taps_of(fmrx, p)
    plain = fmrx.Pipeline(mode, 2, max_block_bytes=nb)
    blocks = []
    for k in range(calls):
        out = plain.process(iq[k * nb:(k + 1) * nb], want_pcm=False)
        r = {t: plain.read_tap(t) for t in ("demod", "stereo_filt", "pll")}
        r.update(audio_l=out["audio_l"], audio_r=out["audio_r"])
        blocks.append(r)
    ovl = fmrx.Pipeline(mode, 2, max_block_bytes=nb)
    ovl.set_option("overlap_calls", lanes)
    na = ovl.n_audio(nb)
    d_iq = torch.from_numpy(iq).cuda()
    outs = [torch.empty(2 * na, dtype=torch.float32, device="cuda") for _ in range(calls)]
    s = torch.cuda.current_stream().cuda_stream
    for k in range(calls):
        ovl.process_dev(d_iq.data_ptr() + k * nb, nb, outs[k].data_ptr(), None, stream=s)
    torch.cuda.synchronize()
    for t in ("demod", "stereo_filt", "pll"):
        bits_equal(ovl.read_tap(t), blocks[-1][t], f"mode {mode} overlap {lanes}: last call's {t}")
    x = concat(blocks, "demod")
    mix = np.concatenate([fm.mixer(b["stereo_filt"], b["pll"]) for b in blocks])
    mono, st = fm.audio_pair(x, mix, h_au, p.audio_decim, (p.stereo_taps - 1) // 2, fm.ascending(p.audio_taps))
    left, right = fm.combine(st, mono)
    tag = f"mode {mode}"
    check_blocks(blocks, "audio_l", left, tag + " plain", fm.combine(fm.ref_chain(mix, h_au, p.audio_decim), mono)[0], True)
    check_blocks(blocks, "audio_r", right, tag + " plain")
    for k in range(calls):
        o = outs[k].cpu().numpy()
        bits_equal(o[:na], left[k * na:(k + 1) * na], f"{tag} overlap_calls {lanes}: left, call {k}")
        bits_equal(o[na:], right[k * na:(k + 1) * na], f"{tag} overlap_calls {lanes}: right, call {k}")


# ---- b. mono, two-kernel path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", AUDIO_SHAPES)
def test_mono_audio_fir_kernel(fmrx, oracle, T, D):
    """audio_fir_kernel behind the mono pipeline of modes 0/1 (fused_min_audio huge: the two-kernel path), the history of
    every block after the first read from the tail of the previous block's buffer (hist_end)."""
    mode = MODE_OF_DECIM[D]
    p = fmrx.modeParams(mode, 101, T)
    h_au = taps_of(fmrx, p)[2]
    cuts = block_cuts(p, False, big=True)
    n = stream_bytes(cuts, p) // 2
    for label, iq, power in (("synthetic", channel_stream(oracle, 2, n, p.rf_Fs), True),
                             ("silence + full scale", silence_then_full_scale(n, n // 3), False)):
        blocks = run_mono(fmrx, p, mode, feed(cuts, p, iq))
        x = concat(blocks, "demod")
        y = fm.fma_chain(x, h_au, fm.polyphase(T, D), D)
        tag = f"mono mode {mode} taps {T} {label}"
        check_blocks(blocks, "audio", y, tag, fm.ref_chain(x, h_au, D), power)
        np.testing.assert_array_equal(concat(blocks, "pcm"), oracle.pcm16(y), tag)
        if not power:
            silent = n // 3 // p.rf_decim - p.rf_taps
            assert not y[:silent // D - T].any()


def run_mono(fmrx, p, mode, blks):
    pl = fmrx.Pipeline(mode, 1, params=p, max_block_bytes=max(len(b) for b in blks))
    pl.set_option("fused_min_audio", 10 ** 12)
    blocks = []
    for blk in blks:
        out = pl.process(blk)
        blocks.append(dict(demod=pl.read_tap("demod"), audio=out["audio"], pcm=out["pcm16"]))
    pl.close()
    return blocks


def test_mono_audio_fir_kernel_persistent_walk(fmrx, oracle):
    """One block of more tiles than audio_fir_kernel launches persistent workgroups (256 x workgroups per CU by its LDS):
    the first workgroups walk a second tile, prefetched while the first one's FMAs run."""
    T, D = 13, 6
    mode = MODE_OF_DECIM[D]
    p = fmrx.modeParams(mode, 101, T)
    wl = D * (256 * 4 - 1) + T                       # AuCfg<T, D, 4, 256>
    lds = ((wl + wl // (4 * D) + 2) * 8 + 15) // 16 * 16
    cap = 256 * min(4, 160 * 1024 // lds)
    n_out = (cap + 64) * 2048 - 5
    cuts = [ref_n_if(p), D * n_out]
    iq = channel_stream(oracle, 3, stream_bytes(cuts, p) // 2, p.rf_Fs)
    blocks = run_mono(fmrx, p, mode, feed(cuts, p, iq))
    x = concat(blocks, "demod")
    h_au = taps_of(fmrx, p)[2]
    check_blocks(blocks, "audio", fm.fma_chain(x, h_au, fm.polyphase(T, D), D), f"mono mode {mode} taps {T}, {cap + 64} tiles",
                 fm.ref_chain(x, h_au, D), True)


# ---- c, d. the fast stereo bank ----------------------------------------------------------------------------------------
def bank_streams(oracle, p, N, n_samples):
    s = [channel_stream(oracle, c, n_samples, p.rf_Fs) for c in range(N)]
    s[1] = silence_then_full_scale(n_samples, n_samples // 3, seed=11)
    return s


def run_bank(fmrx, oracle, mode, taps, N, bb, calls, subset, with_pipelines):
    p = fmrx.modeParams(mode, *taps)
    streams = bank_streams(oracle, p, N, calls * bb // 2)
    ch = fmrx.Channels(mode, N, rf_taps=taps[0], base_audio_taps=taps[1], stereo_taps=taps[2], audio_channels=2, exact=False,
                       block_bytes=bb)
    pls = {}
    if with_pipelines:
        for c in subset:
            pls[c] = fmrx.Pipeline(mode, 2, *taps, max_block_bytes=bb)
            pls[c].set_keep_intermediates(True)
    per = {c: [] for c in subset}
    for k in range(calls):
        out = ch.process(np.stack([s[k * bb:(k + 1) * bb] for s in streams]))
        for c in subset:
            r = {t: ch.read_tap(c, t) for t in ("demod", "stereo_filt", "pll")}
            r.update(audio_l=out["audio_l"][c].copy(), audio_r=out["audio_r"][c].copy(), pcm_l=out["pcm16"][c, :, 0].copy(),
                     pcm_r=out["pcm16"][c, :, 1].copy())
            if c in pls:
                pls[c].process(streams[c][k * bb:(k + 1) * bb], want_pcm=False)
                bits_equal(r["demod"], pls[c].read_tap("demod"), f"bank demod vs single stream, channel {c}, call {k}")
            per[c].append(r)
    ch.close()
    return p, per


@pytest.mark.parametrize("mode,taps,N,per_call", BANK_CONFIGS)
def test_fast_stereo_bank(fmrx, oracle, mode, taps, N, per_call):
    """chs_bpf_kernel and chs_out_kernel (fast bank, modes 0/1) against the model: one block per call (two chunks) and four
    (eight chunks, 65 receivers: two PLL waves), channel 1 on the silence + full-scale stream.  The bank's IF equals the
    single-stream pipeline's (the same matrix-core front end and discriminator)."""
    subset = [c for c in (0, 1, 62, 63, 64) if c < N] + ([N - 1] if N < 63 else [])
    p0 = fmrx.modeParams(mode, *taps)
    bb = per_call * p0.block_bytes
    p, per = run_bank(fmrx, oracle, mode, taps, N, bb, 3, subset, True)
    h_st, _, h_au = taps_of(fmrx, p)
    D, delay = p.audio_decim, (p.stereo_taps - 1) // 2
    for c, blocks in per.items():
        tag = f"fast bank mode {mode} taps {taps} N {N} x {per_call}: channel {c}"
        power = c != 1
        x = concat(blocks, "demod")
        check_blocks(blocks, "stereo_filt", fm.fma_chain(x, h_st, fm.ascending(p.stereo_taps)), tag, fm.ref_chain(x, h_st), power)
        mix = np.concatenate([fm.mixer(b["stereo_filt"], b["pll"]) for b in blocks])
        mono, st = fm.audio_pair(x, mix, h_au, D, delay, fm.ascending(p.audio_taps))
        left, right = fm.combine(st, mono)
        check_blocks(blocks, "audio_l", left, tag, fm.combine(st, fm.ref_chain(x, h_au, D, delay))[0], power)
        check_blocks(blocks, "audio_r", right, tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_l"), oracle.pcm16(left), tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_r"), oracle.pcm16(right), tag)
        if not power:
            silent = len(x) // 3 - p.rf_taps
            assert not x[:silent].any() and not left[:silent // D - p.audio_taps].any()


@pytest.mark.parametrize("mode", [2, 3])
def test_fast_stereo_bank_resampling_modes(fmrx, oracle, mode):
    """Fast bank, modes 2/3: stereo_filt = the ascending chain; L/R = chs_resample_lanes_kernel's model (the reference's
    resampler order, one fma per tap, then y + y U) on the delayed demod stream and on the model's mixer, combined.  It
    differs from the reference's separately rounded resampler (the oracle's convolve_block_resample_fir)."""
    p0 = fmrx.modeParams(mode)
    N = 4
    p, per = run_bank(fmrx, oracle, mode, (101, 101, 101), N, p0.block_bytes, 3, list(range(N)), False)
    h_st, _, h_au = taps_of(fmrx, p)
    delay, n_if, U, D = (p.stereo_taps - 1) // 2, ref_n_if(p), p.audio_upsamp, p.audio_decim
    for c, blocks in per.items():
        tag = f"fast bank mode {mode}: channel {c}"
        power = c != 1
        x = concat(blocks, "demod")
        check_blocks(blocks, "stereo_filt", fm.fma_chain(x, h_st, fm.ascending(p.stereo_taps)), tag, fm.ref_chain(x, h_st), power)
        mix = np.concatenate([fm.mixer(b["stereo_filt"], b["pll"]) for b in blocks])
        left, right = fm.combine(fm.resample_chain(mix, h_au, U, D), fm.resample_chain(x, h_au, U, D, delay))
        # the reference's order with separately rounded products and sums, block by block with its carried state
        xd = np.concatenate([np.zeros(delay, np.float32), x])[:len(x)]
        sm, ss = np.zeros(p.audio_taps - 1, np.float32), np.zeros(p.audio_taps - 1, np.float32)
        mono_r, st_r = [], []
        for b in range(len(blocks)):
            y, sm = oracle.convolve_block_resample_fir(xd[b * n_if:(b + 1) * n_if], h_au, sm, D, U)
            mono_r.append(y)
            y, ss = oracle.convolve_block_resample_fir(mix[b * n_if:(b + 1) * n_if], h_au, ss, D, U)
            st_r.append(y)
        ref_l = fm.combine(np.concatenate(st_r), np.concatenate(mono_r))[0]
        check_blocks(blocks, "audio_l", left, tag, ref_l, power)
        check_blocks(blocks, "audio_r", right, tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_l"), oracle.pcm16(left), tag)
        np.testing.assert_array_equal(concat(blocks, "pcm_r"), oracle.pcm16(right), tag)
