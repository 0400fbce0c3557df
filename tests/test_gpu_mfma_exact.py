"""The f32 matrix-core FIRs checked BIT FOR BIT against the fma-chain models of tests/_fir_model.py, given the input
taps the kernels read:

  mono_fused_kernel (kernels_fe_mfma.hip)       the audio FIR of the mono chain of modes 0/1 = fused_audio: two fmaf
                                                chains (even / odd K-steps) over the Toeplitz tap image, then y0 + y1
  resample_mfma_kernel (kernels_resample.hip)   the resampler of modes 2/3 (mono, and mono_filt / stereo_final of the
                                                stereo chain) = resample_mfma: one fmaf chain per output over the tile's
                                                tap image, then acc + fl(acc U)

Both rest on v_mfma_f32_16x16x4_f32 being a chain of exactly rounded fmaf in K order (MFMA_K_ORDER).  The models are fed
the stream the kernel read, with zeros before its start: the discriminator output of a twin handle that keeps its
intermediates (the fused kernel's own never leaves the chip), or read_tap("demod") / read_tap("mixer") of the same
handle (the resampler).  So a window off by one at a batch, tile or period-block seam, a wrong history sample at the
start of a run or of a block, a tap out of place or a stale staging row changes bits here.  Every block with >= 1000
outputs also has to differ from the other path's model (the two-kernel polyphase chain, the resample_exact twin): the
matrix-core kernel ran.  PCM is the oracle's pcm16 of the model, wrap and saturate, also from PCM-only calls (the
kernels' packed stores)."""
import numpy as np
import pytest

import _fir_model as fm
from test_gpu_channels import channel_stream
from test_gpu_fir_exact import MIN_POWER, bits_equal, concat, differs, offsets, silence_then_full_scale, taps_of

pytestmark = pytest.mark.gpu

# FMRX_FUSED_CASES: (rf taps, rf decim, audio taps, audio decim)
FUSED_CASES = [(101, 10, 101, 5), (151, 10, 101, 5), (13, 10, 101, 5), (101, 10, 13, 5), (151, 10, 13, 5), (13, 10, 13, 5),
               (101, 5, 101, 6), (151, 5, 101, 6), (13, 5, 101, 6), (101, 5, 13, 6), (151, 5, 13, 6), (13, 5, 13, 6)]
MODE_OF_DECIM = {5: 0, 6: 1}
# (mode, base audio taps, periods per call, resample_chains): mono modes 2/3
RESAMPLE_CASES = ([(m, t, n, 0) for m in (2, 3) for t in (101, 13) for n in (64, 64 + 13, 171, 400)]
                  + [(m, t, 1007, c) for m in (2, 3) for t in (101, 13) for c in (1, 2)]
                  + [(2, 101, 2500, 0), (3, 101, 1200, 0)])
# (mode, base audio taps, stereo taps): all-pass delays 50, 6, 75 -- none a multiple of 4
STEREO_RS_CASES = [(m, 101, s) for m in (2, 3) for s in (101, 13, 151)] + [(m, 13, 13) for m in (2, 3)]


def fused_blocks(DA):
    """Audio outputs per block: the first block of the stream (one batch), partial batches, several waves (runs that
    start with a dry tile), carried blocks.  Multiples of 4: the fused kernel needs 16-byte aligned blocks."""
    return [256, 256 * 7 + 4, 256 * 60 + 100, 256 * 33 + 252, 256 * 2 + 8, 1024]


def run_fused(fmrx, mode, T, TA, blocks, wraps=(True, False)):
    """pf: the fused kernel (f32 audio + PCM); pu: the twin that keeps its intermediates (the discriminator stream);
    pc[w]: PCM-only process_dev calls (the pcm_pack_flat store), wrap / saturate.  -> list of per-block dicts."""
    import torch
    mk = lambda: fmrx.Pipeline(mode, 1, rf_taps=T, base_audio_taps=TA, max_block_bytes=max(len(b) for b in blocks))
    pf, pu = mk(), mk()
    pf.set_option("fused_min_audio", 0)
    pu.set_option("fused_min_audio", 10 ** 12)
    pu.set_keep_intermediates(True)
    pcs = {}
    for w in wraps:
        pcs[w] = mk()
        pcs[w].set_option("fused_min_audio", 0)
    out = []
    for k, blk in enumerate(blocks):
        o = pf.process(blk)
        pu.process(blk, want_pcm=False)
        bits_equal(pf.get_state(), pu.get_state(), f"carried state after block {k}")
        r = dict(audio=o["audio"], pcm=o["pcm16"], demod=pu.read_tap("demod"))
        d_iq = torch.from_numpy(np.ascontiguousarray(blk)).cuda()
        for w, pc in pcs.items():
            d_pcm = torch.full((pc.n_audio(len(blk)),), 0x5A5A, dtype=torch.int16, device="cuda")
            pc.process_dev(d_iq.data_ptr(), len(blk), None, d_pcm.data_ptr(), wrap=w)
            torch.cuda.synchronize()
            r[f"pcm_only_{w}"] = d_pcm.cpu().numpy()
        out.append(r)
    for h in [pf, pu, *pcs.values()]:
        h.close()
    return out


def check_fused(oracle, res, h_au, T, D, TA, DA, tag, power):
    x = concat(res, "demod")
    for b, (lo, hi) in enumerate(offsets(res, "audio")):
        y = fm.fused_audio(x, h_au, DA, lo, hi - lo)
        msg = f"{tag}: block {b} ({hi - lo} outputs)"
        bits_equal(res[b]["audio"], y, msg)
        np.testing.assert_array_equal(res[b]["pcm"], oracle.pcm16(y), msg)
        for w in (True, False):
            if f"pcm_only_{w}" in res[b]:
                np.testing.assert_array_equal(res[b][f"pcm_only_{w}"], oracle.pcm16(y, wrap=w), f"{msg}, PCM only, wrap {w}")
        if power and hi - lo >= MIN_POWER:
            assert differs(y, fm.fma_chain(x, h_au, fm.polyphase(TA, DA), DA, 0, lo, hi - lo)), msg + ": equals the two-kernel chain"
    return x


@pytest.mark.parametrize("T,D,TA,DA", FUSED_CASES)
def test_fused_mono_audio_fir(fmrx, oracle, T, D, TA, DA):
    """mono_fused_kernel's audio FIR, every fused shape, the synthetic FM stream and silence then full scale; f32 audio,
    PCM, and PCM-only calls (wrap and saturate)."""
    mode = MODE_OF_DECIM[DA]
    p = fmrx.modeParams(mode, T, TA)
    assert (p.rf_decim, p.audio_decim) == (D, DA)
    h_au = taps_of(fmrx, p)[2]
    cuts = [2 * D * DA * n for n in fused_blocks(DA)]
    assert all(c % 16 == 0 for c in cuts)
    n = sum(cuts) // 2
    for label, iq, power in (("synthetic", channel_stream(oracle, 4, n, p.rf_Fs), True),
                             ("silence + full scale", silence_then_full_scale(n, n // 3), False)):
        blocks, o = [], 0
        for c in cuts:
            blocks.append(iq[o:o + c])
            o += c
        res = run_fused(fmrx, mode, T, TA, blocks)
        x = check_fused(oracle, res, h_au, T, D, TA, DA, f"fused {T}/{D}/{TA}/{DA} {label}", power)
        if not power:
            silent = n // 3 // D - T
            assert not x[:silent].any()


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_mono_audio_fir_bench_block(fmrx, oracle, mode):
    """A bench-sized block (every wave owns two batches: the straight-line batches run, t_fast1 / fast_last), not a whole
    number of batches, after a reference block, and a carried block behind it."""
    p = fmrx.modeParams(mode)
    D, DA = p.rf_decim, p.audio_decim
    unit = 2 * D * DA * 4
    cuts = [p.block_bytes // unit * unit, 2 * D * DA * 256 * 2200 + unit, 256 * unit]
    n_batches = -(-cuts[1] // (2 * D * DA) // 256)
    assert n_batches > 2048                          # more batches than waves in the largest grid: two per wave
    iq = channel_stream(oracle, 6, sum(cuts) // 2, p.rf_Fs)
    blocks, o = [], 0
    for c in cuts:
        blocks.append(iq[o:o + c])
        o += c
    res = run_fused(fmrx, mode, p.rf_taps, p.audio_taps, blocks, wraps=(True,))
    check_fused(oracle, res, taps_of(fmrx, p)[2], p.rf_taps, D, p.audio_taps, DA, f"fused mode {mode} bench block", True)


# ---- the matrix-core resampler -------------------------------------------------------------------------------------
def resample_blocks(p, periods, calls):
    return [2 * periods * p.audio_decim * p.rf_decim] * calls


@pytest.mark.parametrize("mode,taps,periods,chains", RESAMPLE_CASES)
def test_resampler_mono(fmrx, oracle, mode, taps, periods, chains):
    """resample_mfma_kernel behind the mono pipeline of modes 2/3 (16-byte staging): two or three consecutive calls (carried
    history), f32 audio and PCM, and the PCM-only calls' packed store, wrap and saturate; differs from the
    resample_exact twin's."""
    import torch
    p = fmrx.modeParams(mode, 101, taps)
    U, D = p.audio_upsamp, p.audio_decim
    h_au = taps_of(fmrx, p)[2]
    calls = 2 if periods > 1000 else 3
    nb = resample_blocks(p, periods, calls)[0]
    iq = channel_stream(oracle, 8, calls * nb // 2, p.rf_Fs)
    mk = lambda: fmrx.Pipeline(mode, 1, params=p, max_block_bytes=nb)
    a, ex, pw, ps = mk(), mk(), mk(), mk()
    a.set_keep_intermediates(True)
    ex.set_option("resample_exact", 1)
    for h in (a, pw, ps):
        h.set_option("resample_chains", chains)
    d_iq = torch.from_numpy(iq).cuda()
    res = []
    for k in range(calls):
        blk = iq[k * nb:(k + 1) * nb]
        o, oe = a.process(blk), ex.process(blk)
        r = dict(audio=o["audio"], pcm=o["pcm16"], exact=oe["audio"], demod=a.read_tap("demod"))
        for w, h in ((True, pw), (False, ps)):
            d_pcm = torch.full((h.n_audio(nb),), 0x5A5A, dtype=torch.int16, device="cuda")
            h.process_dev(d_iq.data_ptr() + k * nb, nb, None, d_pcm.data_ptr(), wrap=w)
            torch.cuda.synchronize()
            r[f"pcm_only_{w}"] = d_pcm.cpu().numpy()
        res.append(r)
    for h in (a, ex, pw, ps):
        h.close()
    x = concat(res, "demod")
    tag = f"resampler mode {mode} taps {taps} x {periods} periods, chains {chains}"
    for b, (lo, hi) in enumerate(offsets(res, "audio")):
        assert hi - lo == periods * U
        y = fm.resample_mfma(x, h_au, U, D, 0, lo, hi - lo)
        msg = f"{tag}: call {b}"
        bits_equal(res[b]["audio"], y, msg)
        np.testing.assert_array_equal(res[b]["pcm"], oracle.pcm16(y), msg)
        np.testing.assert_array_equal(res[b]["pcm_only_True"], oracle.pcm16(y, wrap=True), msg + ", PCM only, wrap")
        np.testing.assert_array_equal(res[b]["pcm_only_False"], oracle.pcm16(y, wrap=False), msg + ", PCM only, saturate")
        assert differs(res[b]["audio"], res[b]["exact"]), msg + ": equals the resample_exact twin"


@pytest.mark.parametrize("mode,audio_taps,stereo_taps", STEREO_RS_CASES)
def test_resampler_stereo(fmrx, oracle, mode, audio_taps, stereo_taps):
    """Stereo modes 2/3 on one stream: mono_filt = the resampler on the demod stream `delay` samples back (element
    staging: the delay is not a multiple of 4), stereo_final = the resampler on the mixer (element staging too: the mixer
    buffer has no margins), the mixer tap = fm.mixer, L / R = fm.combine, PCM; differs from the resample_exact twin."""
    p = fmrx.modeParams(mode, 101, audio_taps, stereo_taps)
    U, D, delay = p.audio_upsamp, p.audio_decim, (p.stereo_taps - 1) // 2
    assert delay % 4
    h_au = taps_of(fmrx, p)[2]
    per_call = [64, 77, 171, 64]
    cuts = [2 * n * D * p.rf_decim for n in per_call]
    iq = channel_stream(oracle, 9, sum(cuts) // 2, p.rf_Fs)
    mk = lambda: fmrx.Pipeline(mode, 2, params=p, max_block_bytes=max(cuts))
    a, ex = mk(), mk()
    for h in (a, ex):
        h.set_keep_intermediates(True)
    ex.set_option("resample_exact", 1)
    res, o = [], 0
    for c in cuts:
        blk = iq[o:o + c]
        o += c
        out = a.process(blk)
        ex.process(blk, want_pcm=False)
        r = {t: a.read_tap(t) for t in ("demod", "stereo_filt", "pll", "mixer", "mono_filt", "stereo_final")}
        r.update(audio_l=out["audio_l"], audio_r=out["audio_r"], pcm_l=out["pcm16"][0::2], pcm_r=out["pcm16"][1::2],
                 ex_mono=ex.read_tap("mono_filt"), ex_st=ex.read_tap("stereo_final"))
        res.append(r)
    a.close()
    ex.close()
    tag = f"stereo mode {mode} taps {audio_taps}/{stereo_taps}"
    for b in res:
        bits_equal(b["mixer"], fm.mixer(b["stereo_filt"], b["pll"]), tag + ": mixer tap")
    x, mix = concat(res, "demod"), concat(res, "mixer")
    for b, (lo, hi) in enumerate(offsets(res, "audio_l")):
        msg = f"{tag}: call {b}"
        mono = fm.resample_mfma(x, h_au, U, D, delay, lo, hi - lo)
        st = fm.resample_mfma(mix, h_au, U, D, 0, lo, hi - lo)
        bits_equal(res[b]["mono_filt"], mono, msg + ": mono_filt")
        bits_equal(res[b]["stereo_final"], st, msg + ": stereo_final")
        left, right = fm.combine(st, mono)
        bits_equal(res[b]["audio_l"], left, msg + ": left")
        bits_equal(res[b]["audio_r"], right, msg + ": right")
        np.testing.assert_array_equal(res[b]["pcm_l"], oracle.pcm16(left), msg)
        np.testing.assert_array_equal(res[b]["pcm_r"], oracle.pcm16(right), msg)
        assert differs(res[b]["mono_filt"], res[b]["ex_mono"]) and differs(res[b]["stereo_final"], res[b]["ex_st"]), msg
