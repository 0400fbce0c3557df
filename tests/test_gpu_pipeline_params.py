"""Pipelines at parameters off the reference's grid, against the oracle (tests/_pipeline_cases.py has the table).

csrc/pipeline.hip decides per stage which kernel runs and hands the carried state from one kernel to the next; the rest of the
suite runs it at tap counts {13, 101, 151} and the shipped decimations only.  Here every row mixes specialised and generic
stages, or lands on one of the layout rules (Hd, delay, Ha), and is fed four unequal blocks: a middling one, the shortest the
stages accept (shorter than the discriminator history Hd, so that the next block's history comes from two buffers), one whose
byte count is no multiple of 16 (the front end's generic kernel between specialised ones) and one of about 3 000 IF samples.

Bounds (none of them new):
  * set_force_generic(True) keeps the reference's evaluation order in every stage -> audio, the discriminator output and the
    serialised state (fmrx_pipeline_get_state against the oracle's own vectors) are BIT-EQUAL in every block;
  * default dispatch, mono: assert_audio_close per block and assert_pcm_close over the stream (its "fewer than 1 % differ"
    needs more samples than the 10-audio-sample block has), both from test_gpu_parity.py;
  * default dispatch, stereo: AUDIO_ABS_RMS per channel and block: the streams are 35 ms long, inside the first window of
    DESIGN.md section 2;
  * the row with no specialised stage at all is bit-equal under default dispatch too (stereo: with the serial glibc PLL).
"""
import functools

import numpy as np
import pytest

import _pipeline_cases as pc
from _pipeline_cases import CASES, audio_keys, same_bits
from test_gpu_parity import AUDIO_ABS_RMS, FE_VARIANTS, assert_audio_close, assert_pcm_close, rel_rms, rms

pytestmark = pytest.mark.gpu

ROWS = [(name, ch) for name, (_, _, chs) in CASES.items() for ch in chs]
IDS = [f"{name}-{'mono' if ch == 1 else 'stereo'}" for name, ch in ROWS]
STEREO_TAPS = ("carrier_filt", "stereo_filt", "pll")


@functools.lru_cache(maxsize=None)
def _reference(oracle, name, channels):
    """The oracle's answer to one row, computed once and shared (read only): blocks, per-block outputs, intermediates, states."""
    mode, edits, _ = CASES[name]
    p = pc.oracle_params(oracle, mode, edits)
    blocks = pc.stream(oracle, p, pc.ragged_blocks(p, channels), seed=1000 + sorted(CASES).index(name))
    po = oracle.pipeline_params(p, channels)
    outs, states = [], []
    for blk in blocks:
        o = po.process(blk)
        if channels == 2:
            o.update({k: po.intermediate(k) for k in STEREO_TAPS})
        for v in o.values():
            v.setflags(write=False)
        outs.append(o)
        st = po.get_state()
        st.setflags(write=False)
        states.append(st)
    return p, blocks, outs, states


def _device(fmrx, name, channels, blocks):
    mode, edits, _ = CASES[name]
    return fmrx.Pipeline(params=pc.device_params(fmrx, mode, edits), channels=channels, max_block_bytes=max(len(b) for b in blocks))


def test_block_shapes_reach_what_they_are_for(oracle):
    """The table's blocks do what the module's header says, row by row (a check of the test's own inputs)."""
    for name, ch in ROWS:
        mode, edits, _ = CASES[name]
        p = pc.oracle_params(oracle, mode, edits)
        n = pc.ragged_blocks(p, ch)
        Ha, St1, delay, Hd = pc.layout(p, ch)
        assert len(set(n)) == 4 and max(n) <= 3200 and n[1] >= max(Ha, St1)
        if pc.unit_if(p) < 100:
            assert n[1] < Hd, (name, ch, n, Hd)
            assert n[1] < max(Ha, St1) + pc.unit_if(p)
        if any(pc.bytes_of(p, pc.unit_if(p) * k) % 16 for k in (1, 2, 3)):
            assert pc.bytes_of(p, n[2]) % 16, (name, ch, n)
    p = pc.oracle_params(oracle, *CASES["hd_from_bandpass"][:2])
    Ha, St1, delay, Hd = pc.layout(p, 2)
    assert St1 + 3 > Ha + delay and Hd == (St1 + 3 + 3) // 4 * 4 + 4          # Hd = St + 2, rounded
    assert pc.layout(pc.oracle_params(oracle, *CASES["even_stereo_taps"][:2]), 2)[2] == 49
    assert pc.layout(pc.oracle_params(oracle, *CASES["ratio_3_8"][:2]), 1)[0] == 100


@pytest.mark.parametrize("name,channels", ROWS, ids=IDS)
def test_bit_exact_mode_and_state_layout(fmrx, oracle, name, channels):
    """force_generic: audio and discriminator output equal the oracle's in every block, and so does the serialised state after
    every block -- the read direction of the layout include/fmrx.h promises, for every vector of it."""
    p, blocks, outs, states = _reference(oracle, name, channels)
    pl = _device(fmrx, name, channels, blocks)
    pl.set_force_generic(True)
    assert len(pl.get_state()) == pc.state_size(p, channels)
    for b, (blk, ref, st) in enumerate(zip(blocks, outs, states)):
        out = pl.process(blk)
        tag = f"{name}, {channels} ch, block {b} ({len(blk)} bytes)"
        for k in audio_keys(channels):
            same_bits(out[k], ref[k], f"{k} {tag}")
        same_bits(pl.read_tap("demod"), ref["demod"], "demod " + tag)
        same_bits(pl.get_state(), st, "state " + tag)
    pl.close()


@pytest.mark.parametrize("fe", FE_VARIANTS)
@pytest.mark.parametrize("name,channels", ROWS, ids=IDS)
def test_default_dispatch(fmrx, oracle, name, channels, fe):
    p, blocks, outs, states = _reference(oracle, name, channels)
    pl = _device(fmrx, name, channels, blocks)
    pl.set_option("fe_variant", fe)
    worst = dict.fromkeys(audio_keys(channels), 0.0)
    stage = {}
    got_pcm, failures = [], []
    for b, (blk, ref) in enumerate(zip(blocks, outs)):
        out = pl.process(blk)
        tag = f"{name}, {channels} ch, {fe}, block {b} ({len(blk)} bytes)"
        # which stage an error comes from: the taps against the oracle's (printed; the bounds are on the audio)
        stage[b] = {"demod": rel_rms(pl.read_tap("demod"), ref["demod"])}
        if channels == 2:
            stage[b].update({k: rel_rms(pl.read_tap(k), ref[k]) for k in ("carrier_filt", "stereo_filt")})
            stage[b]["pll max abs"] = float(np.abs(pl.read_tap("pll") - ref["pll"]).max())
        for k in audio_keys(channels):
            err = rms(out[k].astype(np.float64) - ref[k])
            worst[k] = max(worst[k], err)
            try:
                if channels == 1:
                    assert_audio_close(out[k], ref[k], tag)
                else:
                    assert err <= AUDIO_ABS_RMS, (k, tag, err)
            except AssertionError as e:
                failures.append(str(e))
        got_pcm.append(out["pcm16"])
    print(f"{name} {channels} ch {fe}: worst rms error per block " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" (bound {AUDIO_ABS_RMS:.0e}" + (", and 1e-5 of the signal's rms)" if channels == 1 else ")"))
    for b, s in stage.items():
        print(f"    block {b}: " + ", ".join(f"{k} {v:.2e}" for k, v in s.items()))
    assert not failures, failures
    if channels == 1:
        assert_pcm_close(np.concatenate(got_pcm), oracle.pcm16(np.concatenate([r["audio"] for r in outs])))
    else:   # interleaved L,R (project.cpp:292-302), from the device's own audio: the PLL's grid steps are not PCM's to answer for
        pcm = np.concatenate(got_pcm)
        assert len(pcm) == 2 * sum(len(r["audio_l"]) for r in outs)
    pl.close()


@pytest.mark.parametrize("fe", FE_VARIANTS)
@pytest.mark.parametrize("channels", [1, 2])
def test_all_generic_row_is_bit_exact_under_default_dispatch(fmrx, oracle, channels, fe):
    """No specialised kernel exists for rf 64 / audio 51 / stereo 75 taps: default dispatch has nothing to choose, so nothing may
    differ from the oracle (stereo: once the PLL is the serial recurrence with glibc's functions, pll_mode 2)."""
    p, blocks, outs, states = _reference(oracle, "all_generic", channels)
    pl = _device(fmrx, "all_generic", channels, blocks)
    pl.set_option("fe_variant", fe)
    if channels == 2:
        pl.set_option("pll_mode", 2)
    for b, (blk, ref, st) in enumerate(zip(blocks, outs, states)):
        out = pl.process(blk)
        tag = f"all generic, {channels} ch, {fe}, block {b}"
        for k in audio_keys(channels):
            same_bits(out[k], ref[k], f"{k} {tag}")
        for i, k in enumerate(audio_keys(channels)):
            np.testing.assert_array_equal(out["pcm16"][i::channels], oracle.pcm16(ref[k]), err_msg=f"pcm {k} {tag}")
        same_bits(pl.read_tap("demod"), ref["demod"], "demod " + tag)
        same_bits(pl.get_state(), st, "state " + tag)
    pl.close()


@pytest.mark.parametrize("channels", [1, 2])
def test_taps_no_multiple_of_upsamp_are_refused(fmrx, oracle, channels):
    """audio_upsamp = 3, audio_taps = 100: the reference's resampler writes its state in slots 2, 5, ... (src/filter.cpp:218-222)
    and reads slots 99 - 3 d = 0 mod 3 (:207), which nothing ever writes: its output depends on where the blocks are cut (shown
    below on the oracle), so no stream can equal it.  fmrx_pipeline_create and the banks refuse such parameters."""
    mode, edits = pc.NOT_A_STREAM
    p = pc.oracle_params(oracle, mode, edits)
    iq = oracle.synth_fm_u8(10 * 8 * 600, rf_Fs=float(p.rf_Fs), seed=3)
    cut = pc.bytes_of(p, 8 * 250)
    whole = oracle.pipeline_params(p, channels).process(iq)["audio_l"]
    h = oracle.pipeline_params(p, channels)
    assert not np.array_equal(whole, np.concatenate([h.process(iq[:cut])["audio_l"], h.process(iq[cut:])["audio_l"]]))
    with pytest.raises(fmrx.FmrxError, match="multiple of audio_upsamp") as e:
        fmrx.Pipeline(params=pc.device_params(fmrx, mode, edits), channels=channels, max_block_bytes=len(iq))
    assert e.value.code == fmrx.EINVAL
    for exact in (True, False):
        with pytest.raises(fmrx.FmrxError, match="multiple of audio_upsamp") as e:
            fmrx.Channels(params=pc.device_params(fmrx, mode, edits), n_channels=2, audio_channels=channels, exact=exact,
                          block_bytes=pc.bytes_of(p, 8 * 200))
        assert e.value.code == fmrx.EINVAL
    # one tap more or less on either side of a multiple is refused, the multiple itself is taken
    for taps, ok in ((302, False), (303, True), (304, False)):
        q = pc.device_params(fmrx, mode, dict(edits, audio_taps=taps))
        if ok:
            fmrx.Pipeline(params=q, channels=channels, max_block_bytes=len(iq)).close()
        else:
            with pytest.raises(fmrx.FmrxError):
                fmrx.Pipeline(params=q, channels=channels, max_block_bytes=len(iq))
