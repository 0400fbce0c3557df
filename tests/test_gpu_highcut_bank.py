"""The high-cut stage behind a bank, its meters and the blend, on one stream: the chain of tests/test_gpu_blend_bank.py (a wide
capture of three RDS stations over noise -> tuner, 8 channels -> fast stereo bank of mode 0 -> Meters.for_bank ->
Blend.for_bank) with HighCut.for_bank behind it, three calls, out of place.  Channels 0-2 sit on the stations, channel 3 on
station 1 mistuned by 20 kHz, channels 4-7 on empty offsets.  (a) every call's status equals the model stepped on that call's
collected records, every call's output the model on what the blend wrote, bit for bit, with the filter state carried, and the
PCM the oracle's pack of it; (b) with defaults the stations come through untouched and the muted channels stay zero; (c) with
the blend's mute floor at 0.25 the empty channels come out low-passed; (d) a ramp that straddles the stations' quieting
cuts them partly; (e) the fused mono bank keeps no rows: refused; an exact mono bank works, here without a blend in between.
The properties of the capture that (b) relies on are stated on the CPU models in tests/test_highcut_model_host.py."""
import numpy as np
import pytest

import _blend_model as bm
import _highcut_model as hm
import _meters_capture as MC
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu

# the stations' quieting on this capture, from the CPU models (tests/test_highcut_model_host.py prints the range): 45.58 ..
# 48.62 pseudo-dB over the three calls.  A ramp from 40 to 54 dB has all of them inside: openness between 0.39 and 0.62
STRADDLE = dict(hc_lo=40.0, hc_hi=54.0)


def run_chain(fmrx, oracle, bp, hp, audio_channels=2, exact=False, fused_mono=False, with_blend=True):
    with bank_chain(fmrx, oracle, fused_mono, audio_channels, exact) as ch:
        torch, bank, ac, n, d_audio = ch.torch, ch.bank, ch.ac, ch.n, ch.d_audio
        meters = fmrx.Meters.for_bank(bank)
        blend = fmrx.Blend.for_bank(bank, meters, fmrx.BlendParams(**bp)) if with_blend else None
        hc = fmrx.HighCut.for_bank(bank, meters, fmrx.HighCutParams(**hp))
        d_blend = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda") if with_blend else d_audio
        d_out = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda")
        d_pcm = torch.full((N, n, ac), 7, dtype=torch.int16, device="cuda")
        calls, refused = [], None
        for i in ch.calls():
            meters.process_bank(stream=ch.s)
            try:
                if with_blend:
                    blend.process_bank(d_audio.data_ptr(), d_blend.data_ptr(), None, stream=ch.s)
                hc.process_bank(d_blend.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr(), stream=ch.s)
            except fmrx.FmrxError as e:
                refused = e.code
                break
            recs, status = meters.collect(), hc.status()
            ch.stream.synchronize()
            calls.append(dict(recs=recs, status=status, audio=d_audio.cpu().numpy(), blend=d_blend.cpu().numpy(), out=d_out.cpu().numpy(),
                              pcm=d_pcm.cpu().numpy(), diag=hc.diagnostics()))
        ch.stream.synchronize()
        if_Fs, audio_Fs = float(bank.params.if_Fs), float(bank.params.audio_Fs)
        for x in (hc, blend, meters):
            if x is not None:
                x.close()
    return dict(calls=calls, refused=refused, if_Fs=if_Fs, audio_Fs=audio_Fs, ac=ac, n=n)


@pytest.fixture(scope="module")
def stereo_chain(fmrx, oracle):
    return run_chain(fmrx, oracle, bm.params(), {})


def check_against_the_model(oracle, ch, bp, hp, with_blend=True):
    """-> the model's status rows per call"""
    bc = bm.control(bp, ch["if_Fs"])
    c = hm.control(hm.params(**hp), ch["if_Fs"], ch["audio_Fs"])
    bstate, state, filt, segs, missed = bm.fresh(N), hm.fresh(N), None, 0, 0
    assert len(ch["calls"]) == MC.CALLS
    rows = []
    for k, call in enumerate(ch["calls"]):
        assert np.isfinite(call["audio"]).all()
        if with_blend:                     # what the blend wrote is what its own model says (tests/test_gpu_blend_bank.py), here too
            bstate = bm.step_all(bc, call["recs"], bstate)
            assert np.array_equal(call["blend"].view(np.uint32), bm.apply(bstate, call["audio"]).view(np.uint32)), k
        state = hm.step_all(c, call["recs"], state)
        for f in hm.STATUS_DTYPE.names:
            assert call["status"][f].tobytes() == state[f].tobytes(), (k, f, call["status"][f], state[f])
        want, filt, m, s = hm.apply(c, state, call["blend"], filt, hm.BUILTIN_W, hm.BUILTIN_L)
        segs, missed = segs + s, missed + m
        assert np.array_equal(call["out"].view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(call["pcm"].reshape(-1), oracle.pcm16(hm.interleave(want).reshape(-1), True)), k
        assert call["diag"] == {"segments": segs, "missed": missed}, k
        rows.append(state)
    return rows


def test_a_status_audio_and_pcm_equal_the_model(oracle, stereo_chain):
    assert stereo_chain["if_Fs"] == 240000.0 and stereo_chain["audio_Fs"] == 48000.0 and stereo_chain["ac"] == 2 and stereo_chain["n"] == 1920
    check_against_the_model(oracle, stereo_chain, bm.params(), {})


def test_b_stations_come_through_and_muted_channels_stay_zero(stereo_chain):
    for k, call in enumerate(stereo_chain["calls"]):
        st = call["status"]
        print(f"call {k}: quieting {np.round(st['quiet_db'], 2)} pseudo-dB")
        assert np.all(st["open"][:4] == 1.0) and np.all(st["p0"][:4] == 0.0) and np.all(st["p1"][:4] == 0.0), k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32)), k
        assert np.all(st["open"][4:] == 0.0) and np.all(st["p1"][4:] == hm.design(2500.0, 48000.0)[1]), k
        assert np.all(call["out"][4:] == 0.0) and np.all(call["pcm"][4:] == 0), k
        assert np.abs(call["audio"][4:]).max() > 0.01            # what was muted was not silence


def high_band_power(x, fs, f_lo):
    """the power above f_lo of each row, by a plain DFT"""
    n = x.shape[-1]
    t = np.arange(n)
    k = np.arange(int(np.ceil(f_lo * n / fs)), n // 2 + 1)
    E = np.exp(-2j * np.pi * np.outer(k, t) / n)
    return (np.abs(x.astype(np.float64) @ E.T) ** 2).sum(axis=-1)


def test_c_with_a_floor_the_empty_channels_are_low_passed(fmrx, oracle, stereo_chain):
    bp = bm.params(mute_floor=0.25)
    ch = run_chain(fmrx, oracle, bp, {})
    rows = check_against_the_model(oracle, ch, bp, {})
    for k, call in enumerate(ch["calls"]):
        assert np.array_equal(call["audio"].view(np.uint32), stereo_chain["calls"][k]["audio"].view(np.uint32))
        assert np.all(rows[k]["p1"][4:] == hm.design(2500.0, 48000.0)[1]), k
        assert np.abs(call["blend"][4:]).max() > 0.0025
        before, after = high_band_power(call["blend"][4:], ch["audio_Fs"], 8000.0), high_band_power(call["out"][4:], ch["audio_Fs"], 8000.0)
        print(f"call {k}: empty channels' power above 8 kHz, out / in: {np.round(10 * np.log10((after / before).max()), 2)} dB at the most")
        assert np.all(after < before), k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32)), k


def test_d_a_ramp_that_straddles_the_stations_quieting_cuts_them_partly(fmrx, oracle):
    ch = run_chain(fmrx, oracle, bm.params(), STRADDLE)
    rows = check_against_the_model(oracle, ch, bm.params(), STRADDLE)
    p_max = hm.design(2500.0, 48000.0)[1]
    for k, st in enumerate(rows):
        print(f"call {k}: stations' openness {np.round(st['open'][:4], 3)}, poles {st['p1'][:4]}")
        partly = (st["p1"][:4] > 0) & (st["p1"][:4] < p_max)
        assert partly.any(), k
        cut = np.flatnonzero(partly)
        assert not np.array_equal(ch["calls"][k]["out"][cut], ch["calls"][k]["audio"][cut]), k


def test_e_the_fused_mono_bank_is_refused(fmrx, oracle):
    ch = run_chain(fmrx, oracle, bm.params(), {}, fused_mono=True, with_blend=False)
    assert ch["refused"] == fmrx.EINVAL and ch["calls"] == []


def test_e_an_exact_mono_bank_works_without_a_blend(fmrx, oracle):
    hp = dict(cut_max=0.5)
    ch = run_chain(fmrx, oracle, bm.params(), hp, audio_channels=1, exact=True, with_blend=False)
    assert ch["refused"] is None and ch["ac"] == 1
    rows = check_against_the_model(oracle, ch, bm.params(), hp, with_blend=False)
    for k, call in enumerate(ch["calls"]):
        assert np.all(rows[k]["open"][:4] == 1.0) and np.all(rows[k]["open"][4:] == 0.5), k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32))
        assert not np.array_equal(call["out"][4:], call["audio"][4:])
