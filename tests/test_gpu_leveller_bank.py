"""The leveller at the end of the chain of tests/_gain_chain.py (bank -> a gain per channel -> AudioMeters.for_bank ->
Leveller.for_bank, on one stream), 50 calls of 1 920 samples (2 s).  (1) the device chain equals the host chain (collect ->
fmrx_leveller_process) bit for bit, and the control rows equal the model's on the collected records; (2) the ungated channels
end at the target, or at their clamp on its far side, within a tolerance the model gives on the same records; (3) the empty
channel stays gated at gain 1 and silent; (4) no PCM sample of the output wraps, though the loud channels' input lies beyond
what the pack holds."""
import math

import numpy as np
import pytest

import _leveller_model as lm
from _gain_chain import EMPTY, GAINS, HOT, N, gain_chain

pytestmark = pytest.mark.gpu

CALLS, W = 50, 64


def lkfs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0 else -99.0


@pytest.fixture(scope="module")
def chain(fmrx, oracle):
    with gain_chain(fmrx, CALLS, lookahead=W) as ch:
        am, lv, d_audio, d_out, d_pcm = ch.am, ch.lv, ch.d_audio, ch.d_out, ch.d_pcm
        am_out = fmrx.AudioMeters.for_bank(ch.bank)
        host = fmrx.Leveller(ch.bank.params.audio_Fs, N, ch.ac, ch.n, lookahead=W)
        calls = []
        for i in ch.calls():
            lv.process_bank(d_audio.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr(), stream=ch.s)
            am_out.process_bank(d_out.data_ptr(), stream=ch.s)
            recs, _ = am.collect()
            out_recs, _ = am_out.collect()
            ch.stream.synchronize()
            calls.append(dict(recs=recs, out_recs=out_recs, status=lv.status(), audio=d_audio.cpu().numpy(), out=d_out.cpu().numpy(),
                              pcm=d_pcm.cpu().numpy()))
        for c in calls:                                                        # the host chain, from the collected records
            o = host.process(c["recs"], c["audio"])
            c["host_out"], c["host_pcm"], c["host_status"] = o["audio"], o["pcm16"], host.status()
        info = dict(calls=calls, ac=ch.ac, n=ch.n, audio_Fs=float(ch.bank.params.audio_Fs), ceiling=lv.ceiling, latency=lv.latency)
        host.close()
        am_out.close()
    return info


def test_1_the_device_chain_equals_the_host_chain_and_the_model(chain):
    assert chain["n"] == 1920 and chain["ac"] == 2 and chain["latency"] == W - 1 and len(chain["calls"]) == CALLS
    c = lm.control(lm.params())
    state = lm.fresh(N)
    for k, call in enumerate(chain["calls"]):
        assert np.array_equal(call["out"].view(np.uint32), call["host_out"].view(np.uint32)), k
        assert np.array_equal(call["pcm"], call["host_pcm"]), k
        assert call["status"].tobytes() == call["host_status"].tobytes(), k
        state = lm.step_all(c, 2, call["recs"], state)
        for f in ("loud_ms", "gain", "gain0", "gain1", "gated", "calls"):
            assert call["status"][f].tobytes() == state[f].tobytes(), (k, f)


def test_2_ungated_channels_end_at_the_target_within_their_clamp(chain):
    """Per channel, from the model on the collected records: the gain g the last call applied and the lag of the estimate behind
    that call's measurement, |10 log10(ms / loud_ms)|.  The output's loudness is the input's plus 20 log10 g where the limiter
    did nothing; the tolerance is that lag (the target is met for the estimate, not for the call), plus 0.05 dB for what the
    ramp inside the call, the delay of 63 samples against the meters' call-aligned sums and the float32 gain leave on a
    stationary programme."""
    p = lm.params()
    c = lm.control(p)
    last = chain["calls"][-1]
    fs2 = c["fs2"]
    for ch in range(N):
        if ch == EMPTY:
            continue
        st, rec, out = last["status"][ch], last["recs"][ch], last["out_recs"][ch]
        ms_in, ms_out = rec["sum_k2"].sum() / rec["n"] / fs2, out["sum_k2"].sum() / out["n"] / fs2
        assert st["gated"] == 0 and all(call["status"]["gated"][ch] == 0 for call in chain["calls"])
        lag = abs(10 * math.log10(ms_in / st["loud_ms"]))
        tol = lag + 0.05
        gain_db = 20 * math.log10(st["gain"])
        print(f"channel {ch} (x{GAINS[ch]}): in {lkfs(ms_in):.2f} LKFS, gain {gain_db:.2f} dB, out {lkfs(ms_out):.2f} LKFS, estimate lag {lag:.4f} dB, "
              f"limited {int(st['limited'])}, min_code {int(st['min_code'])}")
        if ch == HOT:                                          # 20 dB down is not enough: clamped, and the limiter holds the peaks
            assert st["gain"] == c["g_min"] and st["limited"] > 0 and lkfs(ms_out) <= lkfs(ms_in) - p["max_cut_db"] + tol
            continue
        assert st["limited"] == 0 and st["min_code"] == lm.ONE
        assert abs(lkfs(ms_out) - (lkfs(ms_in) + gain_db)) <= tol
        if c["g_min"] < st["gain"] < c["g_max"]:
            assert abs(lkfs(ms_out) - p["target_lkfs"]) <= tol
        elif st["gain"] == c["g_min"]:
            assert p["target_lkfs"] - tol <= lkfs(ms_out) and abs(gain_db + p["max_cut_db"]) < 1e-9
        else:
            assert lkfs(ms_out) <= p["target_lkfs"] + tol and abs(gain_db - p["max_boost_db"]) < 1e-9
    gains = [float(last["status"]["gain"][ch]) for ch in (0, 1, 2)]
    assert gains[0] > gains[1] >= gains[2]                      # the quiet station above the loud ones (which may share the cut's clamp)
    for a, b in ((0, 5), (1, 6), (2, 7)):                       # the same station twice: the same rows
        assert last["status"][a].tobytes() == last["status"][b].tobytes()
        assert np.array_equal(last["out"][a].view(np.uint32), last["out"][b].view(np.uint32))


def test_3_the_empty_channel_stays_gated_at_gain_1(chain):
    for k, call in enumerate(chain["calls"]):
        st = call["status"][EMPTY]
        assert st["gated"] == 1 and st["gain"] == 1.0 and st["gain0"] == 1.0 and st["gain1"] == 1.0 and st["loud_ms"] == 0.0, k
        assert st["limited"] == 0 and st["min_code"] == lm.ONE and st["calls"] == k + 1
        assert not call["out"][EMPTY].any() and not call["pcm"][EMPTY].any()


def test_4_no_pcm_sample_of_the_output_wraps(chain, oracle):
    c = float(chain["ceiling"])
    assert c < 2.0
    wrapped_in = 0
    for k, call in enumerate(chain["calls"]):
        y = call["out"]
        assert np.isfinite(y).all() and np.abs(y).max() <= c * (1 + 2.0 ** -22), k
        flat = lm.interleave(y).reshape(-1)
        wrap, sat = oracle.pcm16(flat, True), oracle.pcm16(flat, False)
        assert np.array_equal(wrap, sat) and np.array_equal(call["pcm"].reshape(-1), wrap), k
        assert np.abs(call["pcm"].astype(np.int32)).max() <= int(c * 16384 * (1 + 2.0 ** -22)) + 1
        wrapped_in += int(np.count_nonzero(np.abs(call["audio"]) >= 2.0))
    assert wrapped_in > 0                                       # what came in would have wrapped
    hot = np.concatenate([call["out"][HOT] for call in chain["calls"][1:]], axis=1)
    assert np.abs(hot).max() >= c * (1 - 2.0 ** -10)            # held at the ceiling, not muted
