"""The audio meters at the end of the chain, on one stream: the chain of tests/test_gpu_highcut_bank.py (a wide capture of three
RDS stations over noise -> tuner, 8 channels -> fast stereo bank of mode 0 -> Meters.for_bank -> Blend.for_bank ->
HighCut.for_bank) with AudioMeters.for_bank behind the high-cut, three calls.  Channels 0-2 sit on the stations, channel 3 on
station 1 mistuned by 20 kHz, channels 4-7 on empty offsets, which the blend mutes.  (1) every call's records, bins and state
equal the model on what the high-cut wrote; (2) the muted channels read -99 and no overs, the stations a finite loudness and a
correlation in (-1, 1]; (3) behind the fused mono bank of mode 0, where the meters' stages are refused, it works too."""
import numpy as np
import pytest

import _audio_meters_model as am
import _meters_capture as MC
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu


def run_chain(fmrx, oracle, fused_mono=False):
    with bank_chain(fmrx, oracle, fused_mono) as ch:
        torch, bank, ac, n, d_audio = ch.torch, ch.bank, ch.ac, ch.n, ch.d_audio
        meters = blend = hc = None
        if not fused_mono:
            meters = fmrx.Meters.for_bank(bank)
            blend = fmrx.Blend.for_bank(bank, meters)
            hc = fmrx.HighCut.for_bank(bank, meters)
        audio_meters = fmrx.AudioMeters.for_bank(bank)
        loud = fmrx.Loudness.for_meters(audio_meters)
        d_out = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda") if not fused_mono else d_audio
        calls = []
        for i in ch.calls():
            if not fused_mono:
                meters.process_bank(stream=ch.s)
                blend.process_bank(d_audio.data_ptr(), d_audio.data_ptr(), None, stream=ch.s)
                hc.process_bank(d_audio.data_ptr(), d_out.data_ptr(), None, stream=ch.s)
            audio_meters.process_bank(d_out.data_ptr(), stream=ch.s)
            recs, bins = audio_meters.collect()
            loud.push(recs, bins)
            ch.stream.synchronize()
            calls.append(dict(recs=recs, bins=bins, state=audio_meters.state(), out=d_out.cpu().numpy(),
                              levels=[audio_meters.derive(r) for r in recs]))
        audio_Fs = float(bank.params.audio_Fs)
        gated = [loud.read(k) for k in range(N)]
        for x in (loud, audio_meters, hc, blend, meters):
            if x is not None:
                x.close()
    return dict(calls=calls, audio_Fs=audio_Fs, ac=ac, n=n, gated=gated)


@pytest.fixture(scope="module")
def stereo_chain(fmrx, oracle):
    return run_chain(fmrx, oracle)


def check_against_the_model(ch):
    state = am.fresh(N)
    assert len(ch["calls"]) == MC.CALLS
    for k, call in enumerate(ch["calls"]):
        assert np.isfinite(call["out"]).all()
        rec, bins, state = am.walk(ch["audio_Fs"], call["out"], state, am.max_bins(ch["audio_Fs"], ch["n"]))
        assert am.same(call["recs"], rec), k
        assert am.same(call["bins"], bins), k
        got = call["state"]
        assert am.same(got["z"][:, :ch["ac"]], state["z"][:, :ch["ac"]]) and am.same(got["bin_acc"][:, :ch["ac"]], state["bin_acc"][:, :ch["ac"]]), k
        assert np.array_equal(got["bin_fill"].astype(np.int64), state["bin_fill"]), k


def test_1_records_bins_and_state_equal_the_model_on_what_the_high_cut_wrote(stereo_chain):
    assert stereo_chain["audio_Fs"] == 48000.0 and stereo_chain["ac"] == 2 and stereo_chain["n"] == 1920
    check_against_the_model(stereo_chain)
    assert sum(int(c["recs"]["bins_done"][0]) for c in stereo_chain["calls"]) == MC.CALLS * 1920 // 4800


def test_2_muted_channels_read_dead_air_and_stations_read_programme(stereo_chain):
    for k, call in enumerate(stereo_chain["calls"]):
        lv = call["levels"]
        print(f"call {k}: loudness {[round(l['loudness_lkfs'], 2) for l in lv]} LKFS, correlation {[round(l['correlation'], 3) for l in lv[:4]]}, "
              f"peak {[round(l['peak_dbfs'][0], 1) for l in lv[:4]]} dBFS")
        for c in range(4, N):                              # muted: silence
            assert lv[c]["loudness_lkfs"] == -99.0 and lv[c]["rms_dbfs"] == (-99.0, -99.0) and lv[c]["peak_dbfs"] == (-99.0, -99.0)
            assert lv[c]["over_fraction"] == 0.0 and call["recs"]["over"][c].sum() == 0 and lv[c]["correlation"] == 0.0
        for c in range(3):                                 # the stations
            assert -99.0 < lv[c]["loudness_lkfs"] < 99.0 and np.isfinite(lv[c]["loudness_lkfs"])
            assert -1.0 < lv[c]["correlation"] <= 1.0
    g = stereo_chain["gated"]
    assert all(g[c]["blocks"] == 0 and g[c]["momentary"] == -99.0 for c in range(N))      # 120 ms of audio: one bin, no block yet


def test_3_behind_the_fused_mono_bank_of_mode_0(fmrx, oracle):
    ch = run_chain(fmrx, oracle, fused_mono=True)
    assert ch["ac"] == 1 and ch["n"] == 1920
    check_against_the_model(ch)
    for call in ch["calls"]:
        assert np.all(call["recs"]["sum_lr"] == 0) and np.all(call["recs"]["sum_k2"][:, 1] == 0) and np.all(call["bins"][:, 1] == 0)
        for c in range(3):
            assert -99.0 < call["levels"][c]["loudness_lkfs"] < 99.0 and call["levels"][c]["correlation"] == 0.0
