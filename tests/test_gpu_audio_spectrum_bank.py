"""The audio spectrum meter behind a receiver bank, on the bank's stream: the chain of tests/_bank_chain.py (three RDS stations over
noise -> tuner, 8 channels -> a bank of mode 0) with AudioSpectrum.for_bank on the rows the bank wrote, two calls, behind the fast
stereo bank and behind the fused mono bank.  (1) every device record and the state equal the model fed the collected rows, and
the host walk, bit for bit; (2) the levels are those of audio rows: finite, no band above the total, the centroid inside the audio
band."""
import numpy as np
import pytest

import _audio_spectrum_model as sp
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu

CALLS = 2


def run_chain(fmrx, oracle, fused_mono):
    with bank_chain(fmrx, oracle, fused_mono) as ch:
        m = fmrx.AudioSpectrum.for_bank(ch.bank)
        assert (m.n_channels, m.audio_channels, m.n_audio, m.audio_Fs) == (N, ch.ac, ch.n, float(ch.bank.params.audio_Fs))
        assert m.n_bands == 23 and tuple(m.edges) == sp.DEFAULT_EDGES
        calls = []
        for i in ch.calls():
            m.process_bank(ch.d_audio.data_ptr(), stream=ch.s)
            rec = m.collect()
            ch.stream.synchronize()
            calls.append(dict(rec=rec, audio=ch.d_audio.cpu().numpy(), state=m.state()))
            if len(calls) == CALLS:
                break
        ch.stream.synchronize()
        info = dict(calls=calls, ac=ch.ac, n=ch.n, levels=[[m.derive(r) for r in call["rec"]] for call in calls], band_hz=m.band_hz())
        m.close()
    return info


@pytest.fixture(scope="module", params=[False, True], ids=["stereo bank", "fused mono bank"])
def chain(request, fmrx, oracle):
    return run_chain(fmrx, oracle, request.param)


def test_1_every_device_record_equals_the_model_and_the_host_walk(fmrx, chain):
    ac = chain["ac"]
    assert len(chain["calls"]) == CALLS and ac in (1, 2)
    state, st = sp.fresh(N), [None] * N
    for k, call in enumerate(chain["calls"]):
        assert call["audio"].shape == (N, ac, chain["n"])
        want, state = sp.walk(call["audio"], state)
        assert sp.same(call["rec"], want), k
        assert sp.same(call["state"], state), k
        for c in range(N):
            host, st[c] = fmrx.audioSpectrumWalk(call["audio"][c], st[c])
            assert sp.same(call["rec"][c], host), (k, c)
    assert (chain["calls"][-1]["rec"]["frames"] == (CALLS * chain["n"]) // 256 - ((CALLS - 1) * chain["n"]) // 256).all()


def test_2_the_levels_are_those_of_audio_rows(chain):
    ac = chain["ac"]
    assert np.allclose(chain["band_hz"], sp.band_hz())
    for k, call in enumerate(chain["calls"]):
        assert (call["rec"]["frames"] > 0).all() and np.isfinite(call["rec"]["band"]).all(), k
        for c, lv in enumerate(chain["levels"][k]):
            assert (np.abs(lv["total_dbfs"][:ac]) < 99.0).all() and (lv["total_dbfs"][ac:] == -99.0).all(), (k, c)      # (noise channels read above full scale)
            live = lv["total_dbfs"][:ac] > -99.0
            assert ((lv["centroid_hz"][:ac][live] > 0.0) & (lv["centroid_hz"][:ac][live] < 24000.0)).all(), (k, c)
            assert (lv["band_dbfs"][:ac, :23] <= lv["total_dbfs"][:ac, None] + 1e-9).all(), (k, c)
    print("total_dbfs of the last call, row 0: " + ", ".join(f"{lv['total_dbfs'][0]:.1f}" for lv in chain["levels"][-1]))
