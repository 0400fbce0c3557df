"""The true-peak meter at both ends of the audio stages, on one stream: the chain of tests/_gain_chain.py (bank -> a gain per
channel -> AudioMeters.for_bank -> Leveller.for_bank) with one TruePeak on the audio meters' input and one on the leveller's float
output, 12 calls of 1 920 samples.  (1) every device record equals truePeakWalk of the collected rows bit
for bit; (2) true_peak >= peak everywhere; (3) the empty channel reads the floor; (4) how far the limited channel's output true
peak lies above the leveller's ceiling is printed for DESIGN.md section 4.16: the limiter bounds samples, not the waveform
between them, so nothing beyond finiteness is asserted of it."""
import math

import numpy as np
import pytest

import _true_peak_model as tp
from _gain_chain import EMPTY, GAINS, HOT, N, gain_chain

pytestmark = pytest.mark.gpu

CALLS, W = 12, 64


@pytest.fixture(scope="module")
def chain(fmrx):
    with gain_chain(fmrx, CALLS, lookahead=W) as ch:
        lv, d_audio, d_out = ch.lv, ch.d_audio, ch.d_out
        tp_in, tp_out = fmrx.TruePeak.for_bank(ch.bank), fmrx.TruePeak.for_bank(ch.bank, limit=lv.ceiling)
        assert (tp_in.n_channels, tp_in.audio_channels, tp_in.n_audio, tp_in.limit) == (N, ch.ac, ch.n, fmrx.TRUE_PEAK_LIMIT)
        calls = []
        for i in ch.calls():
            tp_in.process_bank(d_audio.data_ptr(), stream=ch.s)
            lv.process_bank(d_audio.data_ptr(), d_out.data_ptr(), ch.d_pcm.data_ptr(), stream=ch.s)
            tp_out.process_bank(d_out.data_ptr(), stream=ch.s)
            rec_in, rec_out = tp_in.collect(), tp_out.collect()
            ch.stream.synchronize()
            calls.append(dict(rec_in=rec_in, rec_out=rec_out, status=lv.status(), audio=d_audio.cpu().numpy(), out=d_out.cpu().numpy()))
        info = dict(calls=calls, ac=ch.ac, n=ch.n, ceiling=np.float32(lv.ceiling), state_in=tp_in.state(), state_out=tp_out.state())
        tp_out.close()
        tp_in.close()
    return info


def test_1_every_device_record_equals_the_host_walk_of_the_collected_rows(fmrx, chain):
    assert chain["n"] == 1920 and chain["ac"] == 2 and len(chain["calls"]) == CALLS
    for rows, recs, limit, state in (("audio", "rec_in", fmrx.TRUE_PEAK_LIMIT, "state_in"), ("out", "rec_out", chain["ceiling"], "state_out")):
        st = [None] * N
        for k, call in enumerate(chain["calls"]):
            for c in range(N):
                want, st[c] = fmrx.truePeakWalk(call[rows][c], st[c], limit)
                assert tp.same(call[recs][c], want), (rows, k, c, call[recs][c], want)
        assert tp.same(chain[state], np.stack(st)), rows
        model, _ = tp.walk(chain["calls"][0][rows], tp.fresh(N), limit)      # and the host walk the model, on the first call
        assert tp.same(chain["calls"][0][recs], model), rows


def test_2_a_true_peak_is_never_below_the_sample_peak(chain):
    for k, call in enumerate(chain["calls"]):
        for recs, rows in (("rec_in", "audio"), ("rec_out", "out")):
            r = call[recs]
            assert (r["true_peak"] >= r["peak"]).all() and np.isfinite(r["true_peak"]).all() and (r["n"] == chain["n"]).all(), (k, recs)
            if k > 0:                    # the rows' own sample peak, but for the 6 samples of lag at either end of the call
                assert (r["true_peak"] >= np.abs(call[rows][:, :, :-6]).max(axis=2)).all(), (k, recs)


def test_3_the_empty_channel_reads_the_floor(fmrx, chain):
    for k, call in enumerate(chain["calls"]):
        for recs in ("rec_in", "rec_out"):
            r = call[recs][EMPTY]
            assert not r["true_peak"].any() and not r["peak"].any() and not r["over"].any(), (k, recs)
            lv = fmrx.truePeakDerive(r, 2)
            assert lv["max_dbtp"] == -99.0 and lv["true_peak_dbtp"] == (-99.0, -99.0) and lv["over_fraction"] == 0.0


def test_4_the_limited_channels_true_peak_against_the_ceiling(fmrx, chain):
    """A measurement, not a bound: the limiter holds samples under the ceiling, the waveform between them may pass it."""
    c = float(chain["ceiling"])
    worst, overs = 0.0, 0
    assert sum(int(call["status"]["limited"][HOT]) for call in chain["calls"]) > 0      # the limiter did act on it
    for k, call in enumerate(chain["calls"]):
        r = call["rec_out"][HOT]
        assert np.isfinite(r["true_peak"]).all(), k
        assert r["peak"].max() <= c * (1 + 2.0 ** -22)                      # section 4.15's bound, on the samples
        worst = max(worst, float(r["true_peak"].max()))
        overs += int(r["over"].sum())
    above = 20.0 * math.log10(worst / c)
    print(f"limited channel (x{GAINS[HOT]}): ceiling {20 * math.log10(c / 2.0):.2f} dBFS, output true peak {20 * math.log10(worst / 2.0):.3f} dBTP = "
          f"{above:+.3f} dB against the ceiling; {overs} of {2 * CALLS * chain['n']} groups beyond it")
    quiet = max(float(call["rec_out"][1]["true_peak"].max()) for call in chain["calls"])
    print(f"unlimited channel (x{GAINS[1]}): output true peak {20 * math.log10(quiet / 2.0):.3f} dBTP")
    assert math.isfinite(above)
