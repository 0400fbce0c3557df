"""The stereo blend / soft mute stage on the device against its definition (tests/_blend_model.py), bit for bit: status rows,
audio and PCM, through fmrx_blend_process (hand-made records, seeded random audio with samples beyond +-2, +-0, NaN and
+-inf), over the shapes at which the apply kernel takes another path: 16-byte pieces (stereo, n_audio a multiple of 4),
4-byte accesses (mono, other lengths, an unaligned base), one and two groups per lane (n_audio <= 1024 / above), one and two
workgroups per row (n_audio <= 2048 / above), in place and out of place, float only, PCM only and both, wrap and saturate."""
import numpy as np
import pytest

import _blend_model as bm
import _meters_model as mm
from _stage_cases import offset_rows, same_pcm, same_status

pytestmark = pytest.mark.gpu

IF_FS = 240000.0
CALLS = 6
# (n_channels, audio_channels, n_audio, in place, float output, PCM, wrap, parameter set)
CASES = [
    (1, 2, 4, True, True, True, True, "defaults"),
    (3, 2, 1020, False, True, True, False, "floor and slow"),
    (64, 2, 1024, False, True, False, True, "defaults"),
    (65, 2, 1920, True, True, True, True, "defaults"),
    (1000, 2, 1024, False, False, True, False, "defaults"),
    (3, 2, 1920, False, False, True, True, "narrow"),
    (65, 2, 4, True, True, False, False, "floor and slow"),
    (3, 2, 2052, False, True, True, True, "defaults"),        # 513 groups: a second workgroup on the row, 16-byte pieces
    (3, 2, 2050, True, True, True, True, "defaults"),         # the same by 4-byte accesses, the last group cut
    (1, 1, 1, False, True, True, True, "defaults"),
    (3, 1, 5, True, True, True, False, "floor and slow"),
    (64, 1, 1923, False, False, True, True, "defaults"),
    (65, 1, 1923, True, True, False, True, "narrow"),
    (1000, 1, 5, False, True, True, True, "defaults"),
    (3, 1, 4099, False, True, True, False, "defaults"),
]


def case_id(c):
    N, ac, n, ip, f, p, w, ps = c
    return f"{N}x{ac}x{n}-{'inplace' if ip else 'outofplace'}-{'f32' if f else ''}{'pcm' if p else ''}-{'wrap' if w else 'sat'}-{ps.split()[0]}"


def records(c, N, calls=CALLS):
    """[calls][N] meter records: channel i walks the host tests' sequence i mod 5 (cycled, resets left out), every seventh the
    hand-made edge records"""
    seqs = [[r for r in s if r is not None] for s in bm.sequences(c).values()]
    edges = list(bm.hand_made_records().values())
    out = np.zeros((calls, N), mm.METER_DTYPE)
    for i in range(N):
        s = edges[i // 7:] + edges if i % 7 == 6 else seqs[i % len(seqs)]
        for k in range(calls):
            out[k, i] = s[k % len(s)]
    return out


def check_call(oracle, out, status, want_status, audio, wrap, f32, pcm):
    same_status(status, want_status, bm.STATUS_DTYPE.names)
    want = bm.apply(want_status, audio)
    if f32:
        ok = bm.same(out["audio"], want)
        assert ok.all(), (np.argwhere(~ok)[:5], out["audio"][~ok][:5], want[~ok][:5])
    if pcm:
        same_pcm(oracle, out["pcm16"], want, wrap)
    return want


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_six_calls_equal_the_model(fmrx, oracle, case):
    N, ac, n, in_place, f32, pcm, wrap, pset = case
    p = bm.params(**bm.PARAM_SETS[pset])
    c = bm.control(p, IF_FS)
    recs = records(c, N)
    rng = np.random.default_rng(N * 10007 + n)
    blend = fmrx.Blend(IF_FS, N, ac, n, fmrx.BlendParams(**p))
    state = bm.fresh(N)
    moved = 0
    for k in range(CALLS):
        audio = bm.random_rows(rng, N, ac, n)
        out = blend.process(recs[k], audio, want_f32=f32, want_pcm=pcm, wrap=wrap, in_place=in_place)
        state = bm.step_all(c, recs[k], state)
        check_call(oracle, out, blend.status(), state, audio, wrap, f32, pcm)
        moved += int(np.count_nonzero((state["mono0"] != state["mono1"]) | (state["gain0"] != state["gain1"])))
    assert N < 5 or moved > 0          # ramps did cross call boundaries
    blend.close()


def test_reset_of_one_channel_leaves_the_others_unchanged(fmrx, oracle):
    N, ac, n = 5, 2, 1020
    p = bm.params()
    c = bm.control(p, IF_FS)
    recs = records(c, N)
    rng = np.random.default_rng(99)
    audio = [bm.random_rows(rng, N, ac, n) for _ in range(4)]
    a, b = fmrx.Blend(IF_FS, N, ac, n), fmrx.Blend(IF_FS, N, ac, n)
    state = bm.fresh(N)
    for k in range(4):
        if k == 2:
            b.reset(1)
            state[1] = bm.fresh()
        oa, ob = a.process(recs[k], audio[k]), b.process(recs[k], audio[k])
        state = bm.step_all(c, recs[k], state)
        check_call(oracle, ob, b.status(), state, audio[k], True, True, True)
        others = [0, 2, 3, 4]
        assert np.array_equal(oa["audio"][others].view(np.uint32), ob["audio"][others].view(np.uint32))
        assert np.array_equal(oa["pcm16"][others], ob["pcm16"][others])
        assert a.status()[others].tobytes() == b.status()[others].tobytes()
        if k == 2:      # channel 1 fell from full separation in call 1: a ramp without the reset, a first call with it
            sa, sb = a.status()[1], b.status()[1]
            assert sb["calls"] == 1 and sb["mono0"] == sb["mono1"] and sa["calls"] == 3 and sa["mono0"] != sa["mono1"]
    b.reset()
    assert b.status().tobytes() == bm.fresh(N).tobytes()
    for x in (a, b):
        x.close()


def test_66000_channels(fmrx, oracle):
    """more channels than a grid's y holds; 50 distinct records tiled (a first call's status depends on its record alone)"""
    N, ac, n, K = 66000, 2, 8, 50
    p = bm.params()
    c = bm.control(p, IF_FS)
    base = records(c, K, calls=2)[1]
    recs = np.tile(base, (N + K - 1) // K)[:N]
    want_status = np.tile(bm.step_all(c, base, bm.fresh(K)), (N + K - 1) // K)[:N]
    audio = bm.random_rows(np.random.default_rng(66), N, ac, n)
    blend = fmrx.Blend(IF_FS, N, ac, n)
    out = blend.process(recs, audio)
    check_call(oracle, out, blend.status(), want_status, audio, True, True, True)
    blend.close()


@pytest.mark.parametrize("n", [1024, 1920])
def test_an_unaligned_input_gives_the_same_bits(fmrx, oracle, n):
    N, ac = 3, 2
    p = bm.params()
    c = bm.control(p, IF_FS)
    recs = records(c, N)
    rng = np.random.default_rng(n)
    al, un = fmrx.Blend(IF_FS, N, ac, n), fmrx.Blend(IF_FS, N, ac, n)
    state = bm.fresh(N)
    for k in range(3):
        audio = bm.random_rows(rng, N, ac, n)
        oa = al.process(recs[k], offset_rows(audio, 0))
        ou = un.process(recs[k], offset_rows(audio, 4))
        oi = un.process(recs[k], offset_rows(audio, 4), in_place=True) if k == 2 else None
        state = bm.step_all(c, recs[k], state)
        check_call(oracle, oa, al.status(), state, audio, True, True, True)
        assert np.array_equal(oa["audio"].view(np.uint32), ou["audio"].view(np.uint32)) and np.array_equal(oa["pcm16"], ou["pcm16"])
        if oi is not None:      # a fourth call on that handle: only its 4-byte-offset in-place rows are looked at, against the model
            assert oi["audio"].ctypes.data % 16 == 4
            st = bm.step_all(c, recs[k], state)
            check_call(oracle, oi, un.status(), st, audio, True, True, True)
    for x in (al, un):
        x.close()


def test_process_dev_behind_the_meters_and_its_refusals(fmrx, oracle):
    """fmrx_blend_process_dev reads the MPX results where fmrx_meters_process left them; FMRX_EINVAL where that call had no
    discriminator rows, where no call was made, where the channel counts differ, and without any output.  (The first test of
    the suite that touches torch: it pays torch's start-up, about 10 s once per session, whichever test comes first.)"""
    import torch
    N, ac, n = 4, 2, 1920
    rng = np.random.default_rng(12)
    t = np.arange(4096) / IF_FS
    rows = (0.3 * rng.standard_normal((N, 4096))).astype(np.float32)
    rows[0] += (0.1 * np.cos(2 * np.pi * 19000.0 * t)).astype(np.float32)        # a pilot over noise; the others noise of three strengths
    rows[2] *= 0.01
    rows[3] *= 1e-4
    meters, blend = fmrx.Meters(IF_FS, N), fmrx.Blend(IF_FS, N, ac, n)
    audio = bm.random_rows(rng, N, ac, n)
    d_in = torch.from_numpy(audio).cuda()
    d_out, d_pcm = torch.empty_like(d_in), torch.empty(N * n * ac, dtype=torch.int16, device="cuda")     # written whole by the call
    torch.cuda.synchronize()
    with pytest.raises(fmrx.FmrxError) as e:                                      # no meters call yet
        blend.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    assert e.value.code == fmrx.EINVAL
    recs = meters.process(demod=rows)
    blend.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    status = blend.status()
    torch.cuda.synchronize()
    c = bm.control(bm.params(), IF_FS)
    want_status = bm.step_all(c, recs, bm.fresh(N))
    out = dict(audio=d_out.cpu().numpy(), pcm16=d_pcm.cpu().numpy().reshape(N, n, ac))
    check_call(oracle, out, status, want_status, audio, True, True, True)
    assert len(set(status["gain1"].tolist())) > 1
    for bad in (lambda: blend.process_dev(meters, d_in.data_ptr(), None, None),
                lambda: blend.process_dev(meters, None, d_out.data_ptr(), None)):
        with pytest.raises(fmrx.FmrxError) as e:
            bad()
        assert e.value.code == fmrx.EINVAL
    # another channel count, more and fewer, on handles whose last call did measure rows: refused for the count itself
    # (the control kernel would otherwise read another handle's results by this handle's count), nothing changed
    for other_n in (N + 1, N - 1):
        other = fmrx.Meters(IF_FS, other_n)
        fresh = fmrx.Meters(IF_FS, other_n)
        other.process(demod=np.resize(rows, (other_n, rows.shape[1])))
        for m, words in ((other, "channels on device"), (fresh, "no discriminator rows")):
            with pytest.raises(fmrx.FmrxError) as e:
                blend.process_dev(m, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
            assert e.value.code == fmrx.EINVAL and words in str(e.value), (other_n, str(e.value))
        assert blend.status().tobytes() == status.tobytes()
        for m in (other, fresh):
            m.close()
    meters.process(iq=rng.integers(0, 256, (N, 2048), dtype=np.uint8))            # the RF group alone: n_if = 0
    with pytest.raises(fmrx.FmrxError) as e:
        blend.process_dev(meters, d_in.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr())
    assert e.value.code == fmrx.EINVAL
    assert blend.status().tobytes() == status.tobytes()                          # a refused call changes nothing
    for bad in (lambda: fmrx.Blend(IF_FS, 0, 2, 4), lambda: fmrx.Blend(IF_FS, 1, 3, 4), lambda: fmrx.Blend(IF_FS, 1, 2, 0),
                lambda: fmrx.Blend(IF_FS, 1, 2, 4, fmrx.BlendParams(blend_hi=20.0)), lambda: blend.reset(N)):
        with pytest.raises(fmrx.FmrxError) as e:
            bad()
        assert e.value.code == fmrx.EINVAL
    for x in (meters, blend):
        x.close()
