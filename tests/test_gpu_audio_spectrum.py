"""The audio spectrum meter's kernels against the model (tests/_audio_spectrum_model.py), bit for bit in
records and state (any NaN equal to any NaN): random rows over the channel counts, the lengths around the frame, the two-row
tile and the 16-frame tile, at both alignments; special values across frame, tile and call boundaries; one long row through
the tile sums; reset, a second call before collect, the untouched input, the host call, custom bands, the refusals, and a bank
of more channels than a grid's y holds.

One reference per (audio_channels, n_audio): the model walks M channels at once, three calls with the state carried, and channel
c of a handle is given the model's channel c mod M -- the model's channels do not depend on each other."""
import numpy as np
import pytest

import _audio_spectrum_model as sp

pytestmark = pytest.mark.gpu

F32 = np.float32
CHANNELS = (1, 3, 65)
N_AUDIO = (1, 255, 256, 257, 511, 1920, 4095, 4096, 4097, 8195)
POISON = F32(3e38)                      # what lies between the rows and behind the last: a load past n reads infinity or NaN
_refs = {}


def calls_of(n_audio):
    """the three calls' lengths: the handle's n_audio, then two shorter ones (n <= n_audio is allowed)"""
    return (n_audio, max(1, n_audio // 3), max(1, n_audio // 2))


def walked(n_audio):
    """the channels the model walks: fewer for the three longest lengths"""
    return max(CHANNELS) if n_audio <= 1920 else 5


def reference(ac, n_audio):
    """-> per call (rows [M][ac][n], records, the state after)"""
    key = (ac, n_audio)
    if key not in _refs:
        rng = np.random.default_rng(1000 * ac + n_audio)
        M = walked(n_audio)
        state, out = sp.fresh(M), []
        for n in calls_of(n_audio):
            x = (0.9 * rng.standard_normal((M, ac, n))).astype(F32)
            rec, state = sp.walk(x, state)
            out.append((x, rec, state))
        _refs[key] = out
    return _refs[key]


def on_device(torch, x, wide):
    """rows [N][ac][n] -> (tensor, data pointer, pitch, host image): 16-byte aligned rows in a pitch that is a multiple of 4, or the
    base off by one float and an odd pitch; POISON between the rows and behind the last"""
    N, ac, n = x.shape
    pitch = (n + 3) // 4 * 4 + 4 if wide else n + 1 + n % 2
    assert pitch > n and (pitch % 4 == 0 if wide else pitch % 2 == 1)
    host = np.full(N * ac * pitch + 1 + 16, POISON, F32)
    off = 0 if wide else 1
    host[off:off + N * ac * pitch].reshape(N, ac, pitch)[:, :, :n] = x
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, pitch, host


def check(m, rec, state, where=None, pick=None):
    """the handle's records and state against the model's; pick: the model's channel of every channel of the handle"""
    pick = np.arange(m.n_channels) if pick is None else pick
    got = m.collect()
    assert sp.same(got, rec[pick]), (where, got, rec[pick])
    st = m.state()
    assert sp.same(st, state[pick]), where
    return got


@pytest.mark.parametrize("n_audio", N_AUDIO)
@pytest.mark.parametrize("ac", [1, 2])
def test_1_random_rows_equal_the_model(fmrx, ac, n_audio):
    import torch
    assert fmrx.lib.fmrx_audio_spectrum_tile() == sp.TILE and fmrx.lib.fmrx_audio_spectrum_frame() == sp.FRAME
    ref = reference(ac, n_audio)
    for N in CHANNELS:
        pick = np.arange(N) % walked(n_audio)
        for wide in (True, False):
            m = fmrx.AudioSpectrum(N, ac, n_audio)
            for x, rec, state in ref:
                t, ptr, pitch, host = on_device(torch, x[pick], wide)
                m.process_dev(ptr, pitch, x.shape[2])
                where = (N, wide, x.shape[2])
                got = check(m, rec, state, where, pick)
                assert np.isfinite(got["band"]).all(), where                                      # no load past n: POISON would show
                assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)), where      # the input is untouched
            m.close()


@pytest.mark.parametrize("n", [1900, 16 * 256 + 300])
@pytest.mark.parametrize("ac", [1, 2])
def test_2_special_values_across_frame_tile_and_call_boundaries_equal_the_model(fmrx, ac, n):
    """n = 4396: 17 frames, so the second tile starts at frame 16; in each call the edges lie where the open frame's fill puts them"""
    import torch
    N = 5
    rng = np.random.default_rng(20 + ac + n)
    state = sp.fresh(N)
    handles = {wide: fmrx.AudioSpectrum(N, ac, n) for wide in (True, False)}
    sv = np.array([2.0, -2.0, -0.0, 1e-40, -3e-45, 1.17549435e-38, 0.0, -1e-39, 2.0, -2.0, 1e-40, -0.0], F32)
    seen_nan = seen_inf = False
    for call in range(3):
        fill = int(state["fill"][0])
        x = sp.special_rows(rng, N, ac, n)
        edge = 3 * 256 - fill                                              # a frame's first sample, in the row
        x[0, 0, edge - 6:edge + 6] = sv                                    # across a frame edge
        if n > 16 * 256:
            tile = 16 * 256 - fill
            x[0, ac - 1, tile - 6:tile + 6] = sv[::-1]                     # across the tile edge (frame 16)
        x[1, ac - 1, n - 5:] = [1e-40, -2.0, -0.0, 2.0, -3e-45]            # across the call's end
        x[1, 0, :4] = [-2.0, 1e-40, -0.0, 2.0]                             # and its start
        x[2, 0, :] = rng.choice(np.array([1e-40, -3e-45, 1.17549435e-38, -0.0, 0.0, -1e-39], F32), n)      # denormals and zeros alone
        x[-2, ac - 1, n - 3] = np.nan                                      # a NaN in the open frame: the next call completes it
        x[-1, 0, 700], x[-1, 0, 705] = np.inf, -np.inf                     # both signs in one frame
        assert (700 + fill) // 256 == (705 + fill) // 256 and (fill + n) % 256 > 3
        rec, state = sp.walk(x, state)
        for wide, m in handles.items():
            t, ptr, pitch, _ = on_device(torch, x, wide)
            m.process_dev(ptr, pitch, n)
            check(m, rec, state, (call, wide))
        assert np.isfinite(rec["band"][:3]).all() and not np.isfinite(rec["band"][-1, 0, :23]).any()
        assert (rec["band"][2, 0, :23] == 0).all()                         # the denormals' squares underflow
        if call > 0:
            seen_nan |= bool(np.isnan(rec["band"][-2, ac - 1, :23]).all())
        seen_inf |= bool(np.isinf(rec["band"][-1, 0, :23]).any() or np.isnan(rec["band"][-1, 0, :23]).any())
    assert seen_nan and seen_inf
    for m in handles.values():
        m.close()


@pytest.mark.parametrize("wide", [True, False])
def test_3_one_long_row(fmrx, wide):
    """n_channels = 1: 390 frames in 25 tiles, the last with 6 frames, through the tile sums; then 16 frames with a fill"""
    import torch
    n = 100003
    rng = np.random.default_rng(33)
    x = (0.9 * rng.standard_normal((1, 1, n))).astype(F32)
    m = fmrx.AudioSpectrum(1, 1, n)
    state = sp.fresh(1)
    for k in (n, 4097):
        rec, state = sp.walk(x[:, :, :k], state)
        t, ptr, pitch, _ = on_device(torch, x[:, :, :k], wide)
        m.process_dev(ptr, pitch, k)
        check(m, rec, state, k)
    assert rec["n"][0] == 4097 and rec["frames"][0] == (100003 % 256 + 4097) // 256 == 16
    m.close()


def test_4_reset_of_one_channel_leaves_its_neighbours_alone(fmrx):
    N, ac, n = 66, 2, 7                    # no frame completes; fill grows across calls, and reset meets either buffer
    rng = np.random.default_rng(4)
    m = fmrx.AudioSpectrum(N, ac, n)
    state = sp.fresh(N)
    for call, gone in enumerate((1, 64, None, 65)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        rec, state = sp.walk(x, state)
        got = m.process(x)
        assert sp.same(got, rec) and not got["frames"].any() and not got["band"].any(), call
        assert sp.same(m.state(), state), call
        if gone is not None:
            m.reset(gone)
            state[gone] = np.zeros((), sp.AUDIO_SPECTRUM_STATE_DTYPE)
            assert sp.same(m.state(), state), call
    assert sorted(set(state["fill"].tolist())) == [0, 14, 21, 28]
    frames = np.zeros(N, np.int64)
    for call in range(40):                 # until the channels complete their first frames, at their own fills
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        rec, state = sp.walk(x, state)
        assert sp.same(m.process(x), rec) and sp.same(m.state(), state), call
        frames += rec["frames"].astype(np.int64)
    assert (frames == 1).all()
    m.reset()
    st = m.state()
    assert not st["fill"].any() and not st["carry"].any()
    x = np.ones((N, ac, n), F32)
    assert sp.same(m.process(x), sp.walk(x, sp.fresh(N))[0])
    m.close()


def test_5_the_host_call_returns_the_device_calls_bytes(fmrx):
    import torch
    N, ac, n = 65, 2, 1920
    x = reference(ac, n)[0][0][:N]
    a, b = fmrx.AudioSpectrum(N, ac, n), fmrx.AudioSpectrum(N, ac, n)
    rec_h = a.process(x)
    t = torch.from_numpy(x).cuda()
    b.process_dev(t.data_ptr())
    rec_d = b.collect()
    assert rec_h.tobytes() == rec_d.tobytes() and a.state().tobytes() == b.state().tobytes()
    assert sp.same(rec_h, reference(ac, n)[0][1][:N])
    with pytest.raises(fmrx.FmrxError):
        a.process(np.zeros((N, ac, n + 1), F32))     # more than the handle's n_audio
    a.close()
    b.close()


def test_6_a_second_call_before_collect_replaces_the_results(fmrx):
    import torch
    N, ac, n = 3, 2, 4097
    (x0, _, _), (x1, rec1, state1), _ = reference(ac, n)
    m = fmrx.AudioSpectrum(N, ac, n)
    stream = torch.cuda.Stream()
    t0, t1 = torch.from_numpy(x0[:N]).cuda(), torch.from_numpy(np.ascontiguousarray(x1[:N])).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    m.process_dev(t1.data_ptr(), x1.shape[2], x1.shape[2], stream=stream.cuda_stream)
    check(m, rec1[:N], state1[:N])         # the second call's results; the state advanced by both
    stream.synchronize()
    m.close()


def test_7_a_bank_of_66_000_mono_channels(fmrx):
    """more channels than a grid's y or z holds: the rows ride in x.  Channel c carries row c mod 61 of 61 distinct rows (a prime:
    neighbours and grid wrap-arounds differ)"""
    import torch
    N, n, M = 66000, 300, 61
    rng = np.random.default_rng(7)
    pick = np.arange(N) % M
    m = fmrx.AudioSpectrum(N, 1, n)
    state = sp.fresh(M)
    for call in range(2):
        x = (0.9 * rng.standard_normal((M, 1, n))).astype(F32)
        rec, state = sp.walk(x, state)
        t = torch.from_numpy(x[pick]).cuda()
        m.process_dev(t.data_ptr())
        got = m.collect()
        assert sp.same(got, rec[pick]), call
        assert (got["frames"] == 1).all() and (got["band"][:, 0, :23] > 0).all()
    assert sp.same(m.state(), state[pick])
    m.close()


@pytest.mark.parametrize("edges", [(1, 128), tuple(range(1, 32)) + (40, 128), (5, 6, 100)])
def test_8_custom_edges(fmrx, edges):
    import torch
    N, ac, n = 3, 2, 2500                  # 9 frames: a tile of its own per row
    rng = np.random.default_rng(8 + len(edges))
    m = fmrx.AudioSpectrum(N, ac, n, edges=edges)
    assert tuple(m.edges) == edges and m.n_bands == len(edges) - 1 and m.frame == 256 and m.tile == 16
    assert np.array_equal(m.band_hz(), sp.band_hz(edges))
    state = sp.fresh(N)
    for k in (n, 1000):
        x = sp.special_rows(rng, N, ac, k)
        x[1] *= F32(1e-19)                 # bin powers down to the denormal range
        rec, state = sp.walk(x, state, edges)
        t = torch.from_numpy(x).cuda()
        m.process_dev(t.data_ptr(), k, k)
        got = check(m, rec, state, k)
        assert not got["band"][:, :, len(edges) - 1:].any() and (got["band"][:, :, :len(edges) - 1] > 0).all()
        assert got["band"][1].max() < 1e-30
        lv, want = m.derive(got[0]), sp.derive(rec[0], ac, edges)
        for f in want:
            assert np.allclose(lv[f], want[f], rtol=1e-12, atol=0), f
    m.close()


def test_arguments_are_checked(fmrx):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = fmrx.AudioSpectrum(1, 2, 16)
    for args in ((t.data_ptr(), 16, 17), (t.data_ptr(), 8, 16), (t.data_ptr(), 16, 0), (t.data_ptr() + 2, 16, 16), (None, 16, 16)):
        with pytest.raises(fmrx.FmrxError) as e:
            m.process_dev(*args)
        assert e.value.code == fmrx.EINVAL
    with pytest.raises(fmrx.FmrxError):
        m.collect()                                        # no call yet
    with pytest.raises(fmrx.FmrxError):
        m.reset(1)
    with pytest.raises(fmrx.FmrxError):
        m.process(np.zeros((1, 2, 17), F32))
    m.process_dev(t.data_ptr(), 16, 16)                    # and what is accepted still runs
    got = m.collect()
    assert not got["band"].any() and got["frames"][0] == 0 and got["n"][0] == 16 and m.state()["fill"][0] == 16
    m.close()
    for bad in (dict(n_channels=0), dict(audio_channels=3), dict(n_audio=0), dict(n_audio=2 ** 26 + 1), dict(edges=(1, 1)), dict(edges=(0, 4)),
                dict(edges=(1, 129)), dict(edges=(4, 3)), dict(edges=(1,)), dict(edges=tuple(range(1, 35)))):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.AudioSpectrum(**bad)
        assert e.value.code == fmrx.EINVAL
