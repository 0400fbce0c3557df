"""The variable high-cut stage on the device against its definition (tests/_highcut_model.py), bit for bit: status rows, audio,
PCM and the diagnostics' counts, through fmrx_highcut_process, over six calls whose records walk the cut 0 -> partial -> full
-> partial -> 0, with the filter state carried from call to call.  The expected rows come from the model's parallel walk at
the case's lane shape -- which tests/test_highcut_model_host.py shows to return the serial walk's bits -- so that the number
of segments walked again is checked too.  Shapes: rows shorter than, equal to and one longer than a segment, a row with a
second workgroup of segment lanes and a ragged tail, 1 to 1 000 channels (and 66 000 in a test of its own), mono and stereo, in
place and out of place, float only, PCM only and both, wrap and saturate, the built-in lane shape, (64, 64) and (8, 16)."""
import numpy as np
import pytest

import _highcut_model as hm
from _highcut_cases import AUDIO_FS, BUILTIN, CALLS, IF_FS, Model, check_call, inputs, make, records
from _stage_cases import offset_rows

pytestmark = pytest.mark.gpu

# (n_channels, audio_channels, n_audio, in place, float output, PCM, wrap, lane shape, parameter set, input)
CASES = [
    (1, 2, 1, True, True, True, True, BUILTIN, "fast", "noise"),
    (3, 1, 5, False, True, True, False, BUILTIN, "defaults", "noise"),
    (2, 2, 255, False, True, False, True, BUILTIN, "fast", "fixed"),
    (3, 2, 256, True, True, True, True, (64, 64), "fast", "noise"),
    (2, 1, 257, False, False, True, True, BUILTIN, "half and slow", "fixed"),
    (65, 2, 1920, True, True, True, True, BUILTIN, "fast", "noise"),
    (3, 2, 1920, False, True, True, False, (8, 16), "fast", "fixed"),
    (3, 1, 1920, True, False, True, True, (8, 16), "narrow", "noise"),
    (3, 1, 4099, False, True, True, False, (64, 64), "fast", "fixed"),
    (2, 2, 4099, True, True, False, True, BUILTIN, "defaults", "noise"),
    (1, 1, 65 * hm.BUILTIN_L + 3, False, True, True, True, BUILTIN, "fast", "fixed"),   # 66 segments: a second workgroup of lanes, a ragged tail
    (1000, 2, 5, False, True, True, True, BUILTIN, "fast", "noise"),
    (1000, 1, 255, True, False, True, False, (64, 64), "defaults", "noise"),
    (64, 2, 257, False, True, True, True, (8, 16), "fast", "noise"),
]


def case_id(c):
    N, ac, n, ip, f, p, w, sh, ps, inp = c
    return (f"{N}x{ac}x{n}-{'inplace' if ip else 'outofplace'}-{'f32' if f else ''}{'pcm' if p else ''}-{'wrap' if w else 'sat'}-"
            f"W{sh[0]}L{sh[1]}-{ps.split()[0]}-{inp}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_six_calls_equal_the_model(fmrx, oracle, case):
    N, ac, n, in_place, f32, pcm, wrap, shape, pset, kind = case
    p, c, hc = make(fmrx, N, ac, n, pset, shape)
    recs = records(c, N)
    audio = inputs(kind, np.random.default_rng(N * 10007 + n), N, ac, n)
    model = Model(c, N, ac, shape)
    cuts = []
    for k in range(CALLS):
        out = hc.process(recs[k], audio[k], want_f32=f32, want_pcm=pcm, wrap=wrap, in_place=in_place)
        want = model.call(recs[k], audio[k])
        check_call(oracle, out, hc, model, want, wrap, f32, pcm)
        cuts.append(float(model.status["p1"][0]))
    if pset == "fast":       # channel 0: cut 0 -> partial -> full -> partial -> 0
        pm = float(c["p_max"])
        assert cuts[0] == 0.0 and 0.0 < cuts[1] < pm and cuts[2] == pm and 0.0 < cuts[3] < pm and cuts[4] == cuts[5] == 0.0, cuts
    if shape == (8, 16) and n >= 1920:
        assert model.missed > 0            # the repair path was walked, as often as the model walks it
    hc.close()


def test_the_serial_path_gives_the_same_bits(fmrx, oracle):
    N, ac, n = 5, 2, 1923
    p, c, hc = make(fmrx, N, ac, n, "fast", (8, 16))
    recs = records(c, N)
    audio = inputs("fixed", None, N, ac, n)
    model = Model(c, N, ac, (8, 16))
    for k in range(CALLS):
        forced = k in (1, 2, 4)            # in and out of the serial path on one handle: the state is one and the same
        hc.force_serial(forced)
        out = hc.process(recs[k], audio[k])
        want = model.call(recs[k], audio[k], counted=not forced)
        check_call(oracle, out, hc, model, want, True, True, True)
    assert model.missed > 0
    hc.close()


def test_reset_of_one_channel_in_mid_sequence(fmrx, oracle):
    N, ac, n = 5, 2, 1020
    p, c, a = make(fmrx, N, ac, n, "fast")
    b = make(fmrx, N, ac, n, "fast")[2]
    recs = records(c, N)
    audio = inputs("noise", np.random.default_rng(99), N, ac, n, 4)
    model = Model(c, N, ac, BUILTIN)
    for k in range(4):
        if k == 3:                         # channel 0 is at full cut after call 2: a filter state to lose, a ramp to forget
            b.reset(0)
            model.reset(0)
        oa, ob = a.process(recs[k], audio[k]), b.process(recs[k], audio[k])
        want = model.call(recs[k], audio[k])
        check_call(oracle, ob, b, model, want, True, True, True)
        keep = [1, 2, 3, 4]
        assert np.array_equal(oa["audio"][keep].view(np.uint32), ob["audio"][keep].view(np.uint32)) and np.array_equal(oa["pcm16"][keep], ob["pcm16"][keep])
        assert a.status()[keep].tobytes() == b.status()[keep].tobytes()
        if k == 3:
            sa, sb = a.status()[0], b.status()[0]
            assert sb["calls"] == 1 and sb["p0"] == sb["p1"] and sa["calls"] == 4 and sa["p0"] != sa["p1"]
            assert not np.array_equal(oa["audio"][0].view(np.uint32), ob["audio"][0].view(np.uint32))
    b.reset()
    assert b.status().tobytes() == hm.fresh(N).tobytes()
    with pytest.raises(fmrx.FmrxError) as e:
        b.reset(N)
    assert e.value.code == fmrx.EINVAL
    for x in (a, b):
        x.close()


def test_66000_channels(fmrx, oracle):
    """more rows than a grid's y holds; 50 distinct records tiled (a first call's status depends on its record alone)"""
    N, ac, n, K = 66000, 2, 8, 50
    p, c, hc = make(fmrx, N, ac, n, "defaults")
    base = records(c, K, calls=3)[2]
    recs = np.tile(base, (N + K - 1) // K)[:N]
    audio = hm.random_rows(np.random.default_rng(66), N, ac, n)
    model = Model(c, N, ac, BUILTIN)
    out = hc.process(recs, audio)
    model.status = np.tile(hm.step_all(c, base, hm.fresh(K)), (N + K - 1) // K)[:N]
    want, model.state, _, _ = hm.apply(c, model.status, audio, None, *BUILTIN)
    assert len(set(model.status["p1"].tolist())) > 2
    check_call(oracle, out, hc, model, want, True, True, True)
    hc.close()


def test_a_row_4_bytes_off_gives_the_aligned_rows_bits(fmrx, oracle):
    N, ac, n = 3, 2, 1920
    p, c, al = make(fmrx, N, ac, n, "fast")
    un = make(fmrx, N, ac, n, "fast")[2]
    recs = records(c, N)
    audio = inputs("noise", np.random.default_rng(n), N, ac, n, 3)
    model = Model(c, N, ac, BUILTIN)
    for k in range(3):
        oa = al.process(recs[k], offset_rows(audio[k], 0))
        ou = un.process(recs[k], offset_rows(audio[k], 4), in_place=(k == 2))
        want = model.call(recs[k], audio[k])
        check_call(oracle, oa, al, model, want, True, True, True)
        assert k != 2 or ou["audio"].ctypes.data % 16 == 4
        assert np.array_equal(oa["audio"].view(np.uint32), ou["audio"].view(np.uint32)) and np.array_equal(oa["pcm16"], ou["pcm16"])
    for x in (al, un):
        x.close()


def test_process_dev_behind_the_meters_and_its_refusals(fmrx, oracle):
    """fmrx_highcut_process_dev reads the MPX results where fmrx_meters_process left them; FMRX_EINVAL where that call had no
    discriminator rows, where no call was made, where the channel counts differ, and without any output."""
    import torch
    N, ac, n = 4, 2, 1920
    rng = np.random.default_rng(12)
    rows = (0.3 * rng.standard_normal((N, 4096))).astype(np.float32)      # noise of four strengths: cut, partly cut, open, open
    rows[1] *= 0.08
    rows[2] *= 0.01
    rows[3] *= 1e-4
    p, c, hc = make(fmrx, N, ac, n, "defaults")
    meters = fmrx.Meters(IF_FS, N)
    audio = hm.random_rows(rng, N, ac, n)
    d_in = torch.from_numpy(audio).cuda()
    d_out, d_pcm = torch.empty_like(d_in), torch.empty(N * n * ac, dtype=torch.int16, device="cuda")     # written whole by the call
    torch.cuda.synchronize()
    with pytest.raises(fmrx.FmrxError) as e:                                      # no meters call yet
        hc.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    assert e.value.code == fmrx.EINVAL
    recs = meters.process(demod=rows)
    model = Model(c, N, ac, BUILTIN)
    hc.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    status = hc.status()
    torch.cuda.synchronize()
    want = model.call(recs, audio)
    check_call(oracle, dict(audio=d_out.cpu().numpy(), pcm16=d_pcm.cpu().numpy().reshape(N, n, ac)), hc, model, want, True, True, True)
    assert len(set(status["p1"].tolist())) > 1
    hc.process_dev(meters, d_out.data_ptr(), d_out.data_ptr(), None)              # a second call, in place on the device, float only
    second = d_out.cpu().numpy()
    want2 = model.call(recs, want)
    check_call(oracle, dict(audio=second, pcm16=None), hc, model, want2, True, True, False)
    status = hc.status()
    for bad in (lambda: hc.process_dev(meters, d_in.data_ptr(), None, None),
                lambda: hc.process_dev(meters, None, d_out.data_ptr(), None)):
        with pytest.raises(fmrx.FmrxError) as e:
            bad()
        assert e.value.code == fmrx.EINVAL
    for other_n in (N + 1, N - 1):
        other, fresh = fmrx.Meters(IF_FS, other_n), fmrx.Meters(IF_FS, other_n)
        other.process(demod=np.resize(rows, (other_n, rows.shape[1])))
        for m, words in ((other, "channels on device"), (fresh, "no discriminator rows")):
            with pytest.raises(fmrx.FmrxError) as e:
                hc.process_dev(m, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
            assert e.value.code == fmrx.EINVAL and words in str(e.value), (other_n, str(e.value))
        assert hc.status().tobytes() == status.tobytes()
        for m in (other, fresh):
            m.close()
    meters.process(iq=rng.integers(0, 256, (N, 2048), dtype=np.uint8))            # the RF group alone: n_if = 0
    with pytest.raises(fmrx.FmrxError) as e:
        hc.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    assert e.value.code == fmrx.EINVAL
    assert hc.status().tobytes() == status.tobytes()                             # a refused call changes nothing
    assert hc.diagnostics() == {"segments": model.segments, "missed": model.missed}
    for bad in (lambda: fmrx.HighCut(IF_FS, AUDIO_FS, 0, 2, 4), lambda: fmrx.HighCut(IF_FS, AUDIO_FS, 1, 3, 4),
                lambda: fmrx.HighCut(IF_FS, AUDIO_FS, 1, 2, 0), lambda: fmrx.HighCut(IF_FS, AUDIO_FS, 1, 2, 4, fmrx.HighCutParams(fc_min=500.0))):
        with pytest.raises(fmrx.FmrxError) as e:
            bad()
        assert e.value.code == fmrx.EINVAL
    for x in (meters, hc):
        x.close()
