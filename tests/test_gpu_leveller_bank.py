"""The leveller at the end of the chain, on one stream: a fast stereo bank of mode 0 with 8 channels on the same synthetic
programme -> a gain per channel (0.1, 1, 4, 0 = an empty channel, 30, and 0.1, 1, 4 again) -> AudioMeters.for_bank ->
Leveller.for_bank, 50 calls of 1 920 samples (2 s).  (1) the device chain equals the host chain (collect ->
fmrx_leveller_process) bit for bit, and the control rows equal the model's on the collected records; (2) the ungated channels
end at the target, or at their clamp on its far side, within a tolerance the model gives on the same records; (3) the empty
channel stays gated at gain 1 and silent; (4) no PCM sample of the output wraps, though the loud channels' input lies beyond
what the pack holds."""
import importlib
import math

import numpy as np
import pytest

import _leveller_model as lm

pytestmark = pytest.mark.gpu

N, CALLS, W = 8, 50, 64
GAINS = (0.1, 1.0, 4.0, 0.0, 30.0, 0.1, 1.0, 4.0)
BYTES_PER_CALL = 192000             # 96 000 I/Q samples at 2.4 MS/s: 1 920 audio samples at 48 kHz
EMPTY, HOT = 3, 4


def lkfs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0 else -99.0


@pytest.fixture(scope="module")
def chain(fmrx, oracle):
    import torch
    synth = importlib.import_module(fmrx.__name__ + ".synth")
    iq = synth.synth_fm_u8(CALLS * BYTES_PER_CALL // 2)
    bank = fmrx.Channels(0, N, audio_channels=2, exact=False, block_bytes=BYTES_PER_CALL)
    ac, n = bank.audio_channels, bank.n_audio
    am, am_out = fmrx.AudioMeters.for_bank(bank), fmrx.AudioMeters.for_bank(bank)
    lv = fmrx.Leveller.for_bank(bank, am, lookahead=W)
    host = fmrx.Leveller(bank.params.audio_Fs, N, ac, n, lookahead=W)
    d_iq = torch.from_numpy(iq.reshape(CALLS, BYTES_PER_CALL)).cuda()
    d_gain = torch.tensor(GAINS, dtype=torch.float32, device="cuda").reshape(N, 1, 1)
    d_audio = torch.zeros((N, ac, n), dtype=torch.float32, device="cuda")
    d_out = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros((N, n, ac), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    calls = []
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        for i in range(CALLS):
            d_block = d_iq[i].expand(N, BYTES_PER_CALL).contiguous()
            bank.load_dev(d_block.data_ptr(), stream=s)
            bank.process_dev(d_audio.data_ptr(), None, stream=s)
            d_audio.mul_(d_gain)                                           # the stations differ in level
            am.process_bank(d_audio.data_ptr(), stream=s)
            lv.process_bank(d_audio.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr(), stream=s)
            am_out.process_bank(d_out.data_ptr(), stream=s)
            recs, _ = am.collect()
            out_recs, _ = am_out.collect()
            stream.synchronize()
            calls.append(dict(recs=recs, out_recs=out_recs, status=lv.status(), audio=d_audio.cpu().numpy(), out=d_out.cpu().numpy(),
                              pcm=d_pcm.cpu().numpy()))
    for c in calls:                                                        # the host chain, from the collected records
        o = host.process(c["recs"], c["audio"])
        c["host_out"], c["host_pcm"], c["host_status"] = o["audio"], o["pcm16"], host.status()
    info = dict(calls=calls, ac=ac, n=n, audio_Fs=float(bank.params.audio_Fs), ceiling=lv.ceiling, latency=lv.latency)
    for x in (host, lv, am_out, am, bank):
        x.close()
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
