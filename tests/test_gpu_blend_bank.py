"""The blend stage behind a bank and its meters, on one stream: the chain of tests/test_gpu_meters_bank.py (a wide capture of
three RDS stations over noise -> tuner, 8 channels -> fast stereo bank of mode 0 -> Meters.for_bank) with Blend.for_bank
behind it, three calls, out of place.  Channels 0-2 sit on the stations, channel 3 on station 1 mistuned by 20 kHz,
channels 4-7 on empty offsets.  (a) every call's status equals the model stepped on that call's collected records, every
call's output the model on the bank's audio read back, bit for bit, and the PCM the oracle's pack of it; (b) the stations
come through untouched; (c) the empty channels are muted, or, with a floor, mono at the floor; (d) the fused mono bank keeps
no rows: refused; an exact mono bank keeps them: the gain alone.  (b) and (c) are properties of the definition and of the
capture: tests/test_blend_model_host.py states them on the CPU models."""
import numpy as np
import pytest

import _blend_model as bm
import _meters_capture as MC
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu


def run_chain(fmrx, oracle, p, audio_channels=2, exact=False, fused_mono=False):
    with bank_chain(fmrx, oracle, fused_mono, audio_channels, exact) as ch:
        torch, bank, ac, n, d_audio = ch.torch, ch.bank, ch.ac, ch.n, ch.d_audio
        meters = fmrx.Meters.for_bank(bank)
        blend = fmrx.Blend.for_bank(bank, meters, fmrx.BlendParams(**p))
        d_out = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda")
        d_pcm = torch.full((N, n, ac), 7, dtype=torch.int16, device="cuda")
        calls, refused = [], None
        for i in ch.calls():
            meters.process_bank(stream=ch.s)
            try:
                blend.process_bank(d_audio.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr(), stream=ch.s)
            except fmrx.FmrxError as e:
                refused = e.code
                break
            recs, status = meters.collect(), blend.status()
            ch.stream.synchronize()
            calls.append(dict(recs=recs, status=status, audio=d_audio.cpu().numpy(), out=d_out.cpu().numpy(), pcm=d_pcm.cpu().numpy()))
        ch.stream.synchronize()
        if_Fs = float(bank.params.if_Fs)
        for x in (blend, meters):
            x.close()
    return dict(calls=calls, refused=refused, if_Fs=if_Fs, ac=ac, n=n)


@pytest.fixture(scope="module")
def stereo_chain(fmrx, oracle):
    return run_chain(fmrx, oracle, bm.params())


def check_against_the_model(oracle, ch, p):
    c = bm.control(p, ch["if_Fs"])
    state = bm.fresh(N)
    assert len(ch["calls"]) == MC.CALLS
    for k, call in enumerate(ch["calls"]):
        state = bm.step_all(c, call["recs"], state)
        for f in bm.STATUS_DTYPE.names:
            assert call["status"][f].tobytes() == state[f].tobytes(), (k, f, call["status"][f], state[f])
        assert np.isfinite(call["audio"]).all()
        want = bm.apply(state, call["audio"])
        assert np.array_equal(call["out"].view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(call["pcm"].reshape(-1), oracle.pcm16(bm.interleave(want).reshape(-1), True)), k


def test_a_status_audio_and_pcm_equal_the_model(oracle, stereo_chain):
    assert stereo_chain["if_Fs"] == 240000.0 and stereo_chain["ac"] == 2 and stereo_chain["n"] == 1920
    check_against_the_model(oracle, stereo_chain, bm.params())


def test_b_stations_come_through_bit_for_bit(stereo_chain):
    for k, call in enumerate(stereo_chain["calls"]):
        st = call["status"][:4]
        print(f"call {k}: stations' pilot ratio {np.round(st['pilot_db'], 2)}, quieting {np.round(st['quiet_db'], 2)} pseudo-dB")
        assert np.all(st["lamp"] == 1) and np.all(st["sep"] == 1.0) and np.all(st["gain"] == 1.0), k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32)), k


def test_c_empty_channels_are_muted(stereo_chain):
    for k, call in enumerate(stereo_chain["calls"]):
        st = call["status"][4:]
        print(f"call {k}: empty channels' pilot ratio {np.round(st['pilot_db'], 2)}, quieting {np.round(st['quiet_db'], 2)} pseudo-dB")
        assert np.all(st["lamp"] == 0) and np.all(st["sep"] == 0.0) and np.all(st["gain"] == 0.0), k
        assert np.all(call["out"][4:] == 0.0) and np.all(call["pcm"][4:] == 0), k
        assert np.abs(call["audio"][4:]).max() > 0.01            # what was muted was not silence


def test_c_with_a_floor_the_empty_channels_are_mono_at_the_floor(fmrx, oracle, stereo_chain):
    """mute_floor = 0.25.  The ulp is that of 0.25 max(|L|, |R|), the scale of the input: the two outputs differ by the rounding
    error of L - R, which is at that scale (tests/test_blend_model_host.py::test_full_blend_leaves_left_and_right_one_ulp_apart
    derives it and gives the counter-example to reading it at the outputs' own magnitude)."""
    p = bm.params(mute_floor=0.25)
    ch = run_chain(fmrx, oracle, p)
    check_against_the_model(oracle, ch, p)
    for k, call in enumerate(ch["calls"]):
        assert np.array_equal(call["audio"].view(np.uint32), stereo_chain["calls"][k]["audio"].view(np.uint32))
        st = call["status"][4:]
        assert np.all(st["lamp"] == 0) and np.all(st["sep"] == 0.0) and np.all(st["gain"] == 0.25), k
        L, R = call["audio"][4:, 0].astype(np.float64), call["audio"][4:, 1].astype(np.float64)
        ulp = np.spacing((0.25 * np.maximum(np.abs(L), np.abs(R))).astype(np.float32)).astype(np.float64)
        o = call["out"][4:].astype(np.float64)
        apart = np.abs(o[:, 0] - o[:, 1]) / ulp
        off = np.maximum(np.abs(o[:, 0] - 0.25 * (L + R) / 2), np.abs(o[:, 1] - 0.25 * (L + R) / 2)) / ulp
        print(f"call {k}: L' and R' at most {apart.max():.3f} ulp apart, at most {off.max():.3f} ulp from 0.25 (L + R) / 2")
        assert apart.max() <= 1.0 and off.max() <= 1.0, k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32)), k


def test_d_the_fused_mono_bank_is_refused(fmrx, oracle):
    ch = run_chain(fmrx, oracle, bm.params(), fused_mono=True)
    assert ch["refused"] == fmrx.EINVAL and ch["calls"] == []


def test_d_an_exact_mono_bank_takes_the_gain_alone(fmrx, oracle):
    p = bm.params(mute_floor=0.5)
    ch = run_chain(fmrx, oracle, p, audio_channels=1, exact=True)
    assert ch["refused"] is None and ch["ac"] == 1
    check_against_the_model(oracle, ch, p)
    for k, call in enumerate(ch["calls"]):
        g = call["status"]["gain"]
        assert np.all(g[:4] == 1.0) and np.all(g[4:] == 0.5), k
        assert np.array_equal(call["out"][:4].view(np.uint32), call["audio"][:4].view(np.uint32))
        assert np.array_equal(call["out"][4:], (np.float32(0.5) * call["audio"][4:]).astype(np.float32))
