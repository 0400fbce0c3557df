"""The loudness leveller / peak limiter on the device against its definition (tests/_leveller_model.py), bit for bit: status
rows (min_code and limited included), audio and PCM, through fmrx_leveller_process (hand-made audio meter records; rows with
over-ceiling bursts at the tile's and the call's edges, a NaN and an infinity), over the shapes at which the apply kernel
takes another path: 16-byte pieces (stereo, n_audio a multiple of 4, aligned rows) and 4-byte accesses (mono, other lengths,
a base offset by 4 bytes), calls shorter than the carried state (n_audio < 2W - 2), one workgroup per row and several (n_audio
around the tile length T = fmrx_leveller_tile), every look-ahead's extremes, float only, PCM only and both, wrap and
saturate.  Three successive calls each, so that the state crosses calls at every length.  The model's answer to a shape is
computed once and shared by the cases that differ only in alignment."""
import functools
import math

import numpy as np
import pytest

import _leveller_model as lm
from _stage_cases import offset_rows, same_pcm, same_status

pytestmark = pytest.mark.gpu

F32 = np.float32
CALLS = 3
LOOKAHEADS = (8, 64, 128)
CHANNELS = (1, 3, 65)
OUTPUTS = ("both", "f32", "pcm")
# "hot": a full scale of 4 puts the ceiling at 3.57, beyond what the PCM pack holds, so that wrap and saturate differ
PARAM_SETS = {"defaults": {}, "hot": dict(full_scale=4.0, target_lkfs=-14.0, attack=1.0, release=0.5),
              "limiter": dict(max_boost_db=0.0, max_cut_db=0.0)}


def lengths(W):
    T = 2048 - 2 * W
    return (1, W - 1, 2 * W - 2, 2 * W - 1, T - 1, T, T + 1, 2 * T + 3, 1920)


def records(c, N, ac, n, calls=CALLS):
    """[calls][N] audio meter records: loudness that moves the gain up and down, dead air, a NaN"""
    walk = (-30.0, -12.0, -26.0, -70.0, -23.0, -5.0, -45.0)
    out = np.zeros((calls, N), lm.AUDIO_METER_DTYPE)
    for i in range(N):
        for k in range(calls):
            out[k, i] = lm.rec_for(c, walk[(2 * i + 3 * k + i // 7) % len(walk)], n, ac)
            if i % 11 == 5 and k == 1:
                out[k, i]["sum_k2"][0] = math.nan
    return out


@functools.lru_cache(maxsize=None)
def reference(W, n, ac, N, pset):
    """the inputs of a shape's three calls and the model's outputs and status rows"""
    p = lm.params(**PARAM_SETS[pset])
    c = lm.control(p)
    T = 2048 - 2 * W
    rng = np.random.default_rng(100003 * W + 17 * n + 5 * ac + N)
    recs = records(c, N, ac, n)
    state, lim = lm.fresh(N), [lm.fresh_state(ac, W) for _ in range(N)]
    calls = []
    for k in range(CALLS):
        audio = np.stack([lm.special_rows(rng, ac, n, W, T, scale=0.25 * float(c["ceiling"])) for _ in range(N)])
        state = lm.step_all(c, ac, recs[k], state)
        want, state = lm.apply(state, audio, W, c["ceiling"], lim)
        calls.append(dict(recs=recs[k], audio=audio, want=want, status=state.copy()))
    return p, calls


def check_call(oracle, out, status, call, wrap, outputs):
    same_status(status, call["status"], lm.STATUS_DTYPE.names)
    want = call["want"]
    if outputs != "pcm":
        ok = lm.same(out["audio"], want)
        assert ok.all(), (np.argwhere(~ok)[:5], out["audio"][~ok][:5], want[~ok][:5])
    else:
        assert out["audio"] is None
    if outputs != "f32":
        same_pcm(oracle, out["pcm16"], want, wrap)
    else:
        assert out["pcm16"] is None


def cases():
    out = []
    for wi, W in enumerate(LOOKAHEADS):
        for ni, n in enumerate(lengths(W)):
            for ac in (1, 2):
                for off in (0, 4):
                    i = ni + wi + ac
                    out.append((W, n, ac, CHANNELS[i % 3], off, OUTPUTS[(ni + 2 * wi + ac + off // 4) % 3], bool((ni + wi + off // 4) % 2),
                                "hot" if (ni + ac) % 3 == 0 else "defaults"))
    return out


def case_id(c):
    W, n, ac, N, off, outputs, wrap, pset = c
    return f"W{W}-{N}x{ac}x{n}-at{off}-{outputs}-{'wrap' if wrap else 'sat'}-{pset}"


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_three_calls_equal_the_model(fmrx, oracle, case):
    W, n, ac, N, off, outputs, wrap, pset = case
    assert fmrx.levellerTile(W) == 2048 - 2 * W
    p, calls = reference(W, n, ac, N, pset)
    lv = fmrx.Leveller(48000.0, N, ac, n, fmrx.LevellerParams(**p), lookahead=W)
    assert lv.latency == W - 1 and lv.tile == 2048 - 2 * W and lv.ceiling == lm.control(p)["ceiling"]
    limited = 0
    for call in calls:
        out = lv.process(call["recs"], offset_rows(call["audio"], off), want_f32=outputs != "pcm", want_pcm=outputs != "f32", wrap=wrap)
        check_call(oracle, out, lv.status(), call, wrap, outputs)
        limited += int(call["status"]["limited"].sum())
    assert limited > 0
    lv.close()


def test_wrap_and_saturate_differ_only_beyond_the_pack(fmrx, oracle):
    """the "hot" ceiling lies beyond +-2: the two policies give other PCM there, each the library's pack of the model's floats;
    under the default ceiling no sample can wrap and they agree"""
    W, n, ac, N = 64, 1920, 2, 3
    for pset, differ in (("hot", True), ("defaults", False)):
        p, calls = reference(W, n, ac, N, pset)
        a, b = (fmrx.Leveller(48000.0, N, ac, n, fmrx.LevellerParams(**p), lookahead=W) for _ in range(2))
        seen = False
        for call in calls:
            ow, os_ = a.process(call["recs"], call["audio"], wrap=True), b.process(call["recs"], call["audio"], wrap=False)
            check_call(oracle, ow, a.status(), call, True, "both")
            check_call(oracle, os_, b.status(), call, False, "both")
            seen = seen or not np.array_equal(ow["pcm16"], os_["pcm16"])
            if not differ:
                fin = np.isfinite(call["want"])
                assert np.abs(call["want"][fin]).max() < 2.0
        assert seen == differ
        for x in (a, b):
            x.close()


@pytest.mark.parametrize("W", LOOKAHEADS)
def test_special_rows_across_tiles_and_calls(fmrx, oracle, W):
    """2T + 3 samples per call: bursts on the last sample of a tile and the first of the next, on the call's first and last
    sample (their look-ahead reaches into the neighbouring tile and the next call), a NaN and an infinity"""
    T = fmrx.levellerTile(W)
    n, ac, N = 2 * T + 3, 2, 3
    p, calls = reference(W, n, ac, N, "limiter")
    c = lm.control(p)["ceiling"]
    lv = fmrx.Leveller(48000.0, N, ac, n, fmrx.LevellerParams(**p), lookahead=W)
    for k, call in enumerate(calls):
        out = lv.process(call["recs"], call["audio"])
        check_call(oracle, out, lv.status(), call, True, "both")
        x, y, d = call["audio"], out["audio"], W - 1
        assert (call["status"]["min_code"] == 0).all() and np.isnan(y).sum() == 2 * N              # the NaN, and infinity times 0
        assert (call["status"]["gain0"] == 1).all() and (call["status"]["gain1"] == 1).all()
        fin = np.isfinite(y)
        assert np.abs(y[fin]).max() <= float(c) * (1 + 2.0 ** -22)
        for edge in (0, T - 1, T):                                # a burst beyond the ceiling went in there and came out under it, W - 1 later
            assert np.all(np.abs(x[:, :, edge]).max(axis=1) > c) and np.all(np.abs(y[:, :, edge + d]).max(axis=1) > 0.1 * float(c)), (k, edge)
        if k:                                                     # the last call's last sample comes out of this one
            assert np.all(np.abs(calls[k - 1]["audio"][:, :, n - 1]).max(axis=1) > c) and np.all(np.abs(y[:, :, d - 1]).max(axis=1) > 0.1 * float(c))
    lv.close()


def test_reset_of_one_channel_leaves_the_others_unchanged(fmrx, oracle):
    W, n, ac, N = 64, 1920, 2, 5
    p, calls = reference(W, n, ac, N, "defaults")
    calls = calls + calls[:1]
    c = lm.control(p)
    a, b = fmrx.Leveller(48000.0, N, ac, n, lookahead=W), fmrx.Leveller(48000.0, N, ac, n, lookahead=W)
    state, lim = lm.fresh(N), [lm.fresh_state(ac, W) for _ in range(N)]
    others = [0, 2, 3, 4]
    for k, call in enumerate(calls):
        if k == 2:
            b.reset(1)
            state[1], lim[1] = lm.fresh(), lm.fresh_state(ac, W)
        oa, ob = a.process(call["recs"], call["audio"]), b.process(call["recs"], call["audio"])
        state = lm.step_all(c, ac, call["recs"], state)
        want, state = lm.apply(state, call["audio"], W, c["ceiling"], lim)
        check_call(oracle, ob, b.status(), dict(want=want, status=state), True, "both")
        assert np.array_equal(oa["audio"][others].view(np.uint32), ob["audio"][others].view(np.uint32))
        assert np.array_equal(oa["pcm16"][others], ob["pcm16"][others])
        assert a.status()[others].tobytes() == b.status()[others].tobytes()
        if k == 2:          # the reset channel starts from silence and a first call; the other handle's carries its tail and its ramp
            sa, sb = a.status()[1], b.status()[1]
            assert sb["calls"] == 1 and sb["gain0"] == sb["gain1"] and sa["calls"] == 3
            assert np.all(ob["audio"][1, :, :W - 1] == 0) and np.any(oa["audio"][1, :, :W - 1] != 0)
    b.reset()
    assert b.status().tobytes() == lm.fresh(N).tobytes()
    out = b.process(calls[0]["recs"], calls[0]["audio"])
    check_call(oracle, out, b.status(), reference(W, n, ac, N, "defaults")[1][0], True, "both")       # as a fresh handle's first call
    for x in (a, b):
        x.close()


def test_66000_channels(fmrx, oracle):
    """more channels than a grid's y holds; 40 distinct channels tiled"""
    W, n, ac, K, N = 8, 24, 2, 40, 66000
    p = lm.params()
    c = lm.control(p)
    rng = np.random.default_rng(66)
    recs = records(c, K, ac, n, calls=1)[0]
    audio = np.stack([lm.special_rows(rng, ac, n, W, 11, scale=0.5) for _ in range(K)])
    status = lm.step_all(c, ac, recs, lm.fresh(K))
    want, status = lm.apply(status, audio, W, c["ceiling"], [lm.fresh_state(ac, W) for _ in range(K)])
    reps = (N + K - 1) // K
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:N]
    lv = fmrx.Leveller(48000.0, N, ac, n, lookahead=W)
    out = lv.process(tile(recs), tile(audio))
    check_call(oracle, out, lv.status(), dict(want=tile(want), status=tile(status)), True, "both")
    lv.close()


def test_process_dev_behind_the_audio_meters_and_its_refusals(fmrx, oracle):
    """fmrx_leveller_process_dev reads the sums where fmrx_audio_meters_process_dev left them; FMRX_EINVAL for an audio meters
    handle that has not run, that walked another n, that has another channel count or other rows, for overlapping input and
    output, and without any output.  A refused call changes nothing."""
    import torch
    W, n, ac, N = 64, 1920, 2, 4
    p, calls = reference(W, n, ac, N, "defaults")
    c = lm.control(p)
    am, lv = fmrx.AudioMeters(48000.0, N, ac, n), fmrx.Leveller(48000.0, N, ac, n, lookahead=W)
    audio = calls[0]["audio"].copy()
    audio[np.isnan(audio) | np.isinf(audio)] = 0.5                 # (a NaN would poison the meters' sums: that path is the host test's)
    audio[1] *= F32(0.05)
    audio[2] = 0.0
    d_in = torch.from_numpy(audio).cuda()
    d_out, d_pcm = torch.empty_like(d_in), torch.empty(N * n * ac, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    args = (d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    with pytest.raises(fmrx.FmrxError) as e:                                          # no audio meters call yet
        lv.process_dev(am, *args)
    assert e.value.code == fmrx.EINVAL and "no call" in str(e.value)
    am.process_dev(d_in.data_ptr())
    lv.process_dev(am, *args)
    status = lv.status()
    recs, _ = am.collect()
    torch.cuda.synchronize()
    want_status = lm.step_all(c, ac, recs, lm.fresh(N))
    want, want_status = lm.apply(want_status, audio, W, c["ceiling"], [lm.fresh_state(ac, W) for _ in range(N)])
    out = dict(audio=d_out.cpu().numpy(), pcm16=d_pcm.cpu().numpy().reshape(N, n, ac))
    check_call(oracle, out, status, dict(want=want, status=want_status), True, "both")
    assert status["gated"].tolist() == [0, 0, 1, 0] and len(set(status["gain1"].tolist())) > 2
    size = d_in.numel() * 4
    bad = [lambda: lv.process_dev(am, d_in.data_ptr(), None, None), lambda: lv.process_dev(am, None, d_out.data_ptr(), None),
           lambda: lv.process_dev(am, d_in.data_ptr(), d_in.data_ptr(), None),                                   # in place
           lambda: lv.process_dev(am, d_in.data_ptr(), d_in.data_ptr() + size - 4, None),                        # the last float
           lambda: lv.process_dev(am, d_in.data_ptr() + 4 * n, d_in.data_ptr(), None),                           # shifted by a row
           lambda: lv.process_dev(am, d_in.data_ptr(), None, d_in.data_ptr() + size - 2),                        # the PCM in the input
           lambda: fmrx._check(fmrx.lib.fmrx_leveller_process_dev(lv._h, am._h, d_in.data_ptr(), d_out.data_ptr(), None, 7, None))]   # no such policy
    for f in bad:
        with pytest.raises(fmrx.FmrxError) as e:
            f()
        assert e.value.code == fmrx.EINVAL
    for words, other in (("channels of", fmrx.AudioMeters(48000.0, N + 1, ac, n)), ("channels of", fmrx.AudioMeters(48000.0, N - 1, ac, n)),
                         ("channels of", fmrx.AudioMeters(48000.0, N, 1, n)), ("samples per row", fmrx.AudioMeters(48000.0, N, ac, n))):
        fresh = fmrx.AudioMeters(48000.0, other.n_channels, other.audio_channels, n)
        m = n - 4 if words == "samples per row" else n
        other.process(np.zeros((other.n_channels, other.audio_channels, m), F32))
        for h, w in ((other, words), (fresh, "no call")):
            with pytest.raises(fmrx.FmrxError) as e:
                lv.process_dev(h, *args)
            assert e.value.code == fmrx.EINVAL and w in str(e.value), str(e.value)
        for h in (other, fresh):
            h.close()
    assert lv.status().tobytes() == status.tobytes()                                  # a refused call changes nothing
    x = np.zeros((N, ac, n), F32)
    with pytest.raises(fmrx.FmrxError) as e:                                          # the host call: out over in
        fmrx._check(fmrx.lib.fmrx_leveller_process(lv._h, recs.ctypes.data, x.ctypes.data, x.ctypes.data, None, fmrx.PCM_WRAP))
    assert e.value.code == fmrx.EINVAL
    with pytest.raises(fmrx.FmrxError) as e:                                          # the same through the class: in place
        lv.process(recs, x, in_place=True)
    assert e.value.code == fmrx.EINVAL
    for f in (lambda: fmrx.Leveller(48000.0, 0, 2, 4), lambda: fmrx.Leveller(48000.0, 1, 3, 4), lambda: fmrx.Leveller(48000.0, 1, 2, 0),
              lambda: fmrx.Leveller(48000.0, 1, 2, 4, lookahead=12), lambda: fmrx.Leveller(48000.0, 1, 2, 4, lookahead=256),
              lambda: fmrx.Leveller(1000.0, 1, 2, 4), lambda: fmrx.Leveller(48000.0, 1, 2, 4, fmrx.LevellerParams(ceiling_dbfs=0.0)),
              lambda: lv.reset(N)):
        with pytest.raises(fmrx.FmrxError) as e:
            f()
        assert e.value.code == fmrx.EINVAL
    dflt = fmrx.Leveller(48000.0, 1, 2, 4, lookahead=0)                                # 0: the default look-ahead
    assert dflt.latency == 63
    for x in (dflt, am, lv):
        x.close()
