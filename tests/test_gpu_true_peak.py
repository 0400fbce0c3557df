"""The true-peak meter's kernel against the model (tests/_true_peak_model.py), bit for bit (any NaN equal
to any NaN): random rows over the channel counts, the lengths around the carry and the tile, and both fetch paths; the special
values across tile and call boundaries; one long row; reset, a second call before collect, the untouched input, the host call,
the refusals, and a bank of more channels than a grid's y holds.

One reference per (audio_channels, n_audio): the model walks 65 channels at once, three calls with the state carried, and a
handle of N channels is given the first N of them -- the model's channels do not depend on each other."""
import numpy as np
import pytest

import _true_peak_model as tp

pytestmark = pytest.mark.gpu

F32 = np.float32
T = 2048                                # fmrx_true_peak_tile()
CHANNELS = (1, 3, 65)
N_AUDIO = (1, 10, 11, 12, T - 1, T, T + 1, 2 * T + 3, 1920)
POISON = F32(3e38)                      # what lies between the rows and behind the last: a load past n reads infinity or NaN
_refs = {}


def calls_of(n_audio):
    """the three calls' lengths: the handle's n_audio, then two shorter ones (n <= n_audio is allowed; no multiples of 4)"""
    return (n_audio, max(1, n_audio // 3), max(1, n_audio // 2))


def reference(ac, n_audio):
    """-> per call (rows [65][ac][n], records, the state after)"""
    key = (ac, n_audio)
    if key not in _refs:
        rng = np.random.default_rng(1000 * ac + n_audio)
        state, out = tp.fresh(max(CHANNELS)), []
        for n in calls_of(n_audio):
            x = (0.9 * rng.standard_normal((max(CHANNELS), ac, n))).astype(F32)
            rec, state = tp.walk(x, state)
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


def check(m, rec, state, N, ac, where=None):
    got = m.collect()
    assert tp.same(got, rec[:N]), (where, got, rec[:N])
    assert (got["true_peak"] >= got["peak"]).all(), where
    st = m.state()
    assert tp.same(st[:, :ac], state[:N, :ac]) and not st[:, ac:].any(), where


@pytest.mark.parametrize("n_audio", N_AUDIO)
@pytest.mark.parametrize("ac", [1, 2])
def test_1_random_rows_equal_the_model(fmrx, ac, n_audio):
    import torch
    assert fmrx.lib.fmrx_true_peak_tile() == T
    ref = reference(ac, n_audio)
    for N in CHANNELS:
        for wide in (True, False):
            m = fmrx.TruePeak(N, ac, n_audio)
            for x, rec, state in ref:
                t, ptr, pitch, host = on_device(torch, x[:N], wide)
                m.process_dev(ptr, pitch, x.shape[2])
                where = (N, wide, x.shape[2])
                check(m, rec, state, N, ac, where)
                assert np.isfinite(m.collect()["true_peak"]).all(), where                        # no load past n: POISON would show
                assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)), where      # the input is untouched
            m.close()


@pytest.mark.parametrize("ac", [1, 2])
def test_2_special_values_across_tile_and_call_boundaries_equal_the_model(fmrx, ac):
    import torch
    N, n = 5, 2 * T + 3
    rng = np.random.default_rng(2 + ac)
    state = tp.fresh(N)
    handles = {wide: fmrx.TruePeak(N, ac, n) for wide in (True, False)}
    up, down = np.nextafter(tp.LIMIT, F32(4)), np.nextafter(tp.LIMIT, F32(0))
    for call in range(3):
        x = tp.special_rows(rng, N, ac, n)
        x[0, 0, T - 3:T + 9] = [2.0, -2.0, -0.0, 1e-40, tp.LIMIT, up, down, -up, -3e-45, 0.0, 2.0, -2.0]      # a window on the first tile's edge
        x[1, ac - 1, n - 5:] = [up, 1e-40, -2.0, tp.LIMIT, 2.0]                                               # across the call's end
        x[1, 0, :4] = [-2.0, down, -0.0, up]                                                                  # and its start
        x[-1, 0, 2 * T - 4], x[-1, 0, 2 * T] = np.inf, -np.inf                                                # both signs across the second edge and the call's end
        x[-2, ac - 1, n - 3] = np.nan                                                                         # a NaN whose window the next call ends
        rec, state = tp.walk(x, state)
        for wide, m in handles.items():
            t, ptr, pitch, _ = on_device(torch, x, wide)
            m.process_dev(ptr, pitch, n)
            check(m, rec, state, N, ac, (call, wide))
        assert np.isinf(rec["true_peak"][-1, 0]) and np.isinf(rec["peak"][-1, 0]) and np.isfinite(rec["true_peak"][:3]).all()
        assert rec["over"][:3, :ac].min() > 0 and (rec["over"][:3, :ac] < n).all()
    for m in handles.values():
        m.close()


@pytest.mark.parametrize("wide", [True, False])
def test_3_one_long_row(fmrx, wide):
    """n_channels = 1: 49 tiles, the last with 1 699 samples"""
    import torch
    n = 100003
    rng = np.random.default_rng(33)
    x = (0.9 * rng.standard_normal((1, 1, n))).astype(F32)
    x[0, 0, 60000], x[0, 0, 99999] = 3.5, -2.5
    m = fmrx.TruePeak(1, 1, n)
    state = tp.fresh(1)
    for k in (n, 4097):
        rec, state = tp.walk(x[:, :, :k], state)
        t, ptr, pitch, _ = on_device(torch, x[:, :, :k], wide)
        m.process_dev(ptr, pitch, k)
        check(m, rec, state, 1, 1, k)
    assert rec["n"][0] == 4097 and m.collect()["over"][0, 0] == rec["over"][0, 0] > 0
    m.close()


def test_4_reset_of_one_channel_leaves_its_neighbours_alone(fmrx):
    N, ac, n = 66, 2, 7                    # n < 11: the state keeps entries of the call before, and reset meets either buffer
    rng = np.random.default_rng(4)
    m = fmrx.TruePeak(N, ac, n)
    state = tp.fresh(N)
    for call, gone in enumerate((1, 64, None, 65)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        rec, state = tp.walk(x, state)
        got = m.process(x)
        assert tp.same(got, rec), call
        assert tp.same(m.state(), state), call
        if gone is not None:
            m.reset(gone)
            state[gone] = 0
            assert tp.same(m.state(), state), call
    m.reset()
    assert not m.state().any()
    x = np.ones((N, ac, n), F32)
    assert tp.same(m.process(x), tp.walk(x, tp.fresh(N))[0])
    m.close()


def test_5_the_host_call_returns_the_device_calls_bytes(fmrx):
    import torch
    N, ac, n = 65, 2, T + 1
    x = reference(ac, n)[0][0][:N]
    a, b = fmrx.TruePeak(N, ac, n), fmrx.TruePeak(N, ac, n)
    rec_h = a.process(x)
    t = torch.from_numpy(x).cuda()
    b.process_dev(t.data_ptr())
    rec_d = b.collect()
    assert rec_h.tobytes() == rec_d.tobytes() and a.state().tobytes() == b.state().tobytes()
    assert tp.same(rec_h, reference(ac, n)[0][1][:N])
    with pytest.raises(fmrx.FmrxError):
        a.process(np.zeros((N, ac, n + 1), F32))     # more than the handle's n_audio
    a.close()
    b.close()


def test_6_a_second_call_before_collect_replaces_the_results(fmrx):
    import torch
    N, ac, n = 3, 2, 2 * T + 3
    (x0, _, _), (x1, rec1, state1), _ = reference(ac, n)
    m = fmrx.TruePeak(N, ac, n)
    stream = torch.cuda.Stream()
    t0, t1 = torch.from_numpy(x0[:N]).cuda(), torch.from_numpy(np.ascontiguousarray(x1[:N])).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    m.process_dev(t1.data_ptr(), x1.shape[2], x1.shape[2], stream=stream.cuda_stream)
    check(m, rec1, state1, N, ac)          # the second call's results; the state advanced by both
    stream.synchronize()
    m.close()


def test_7_a_bank_of_66_000_mono_channels(fmrx):
    """more channels than a grid's y or z holds: the channel rides in x"""
    import torch
    N, n = 66000, 64
    rng = np.random.default_rng(7)
    m = fmrx.TruePeak(N, 1, n)
    state = tp.fresh(N)
    for call in range(2):
        x = (0.9 * rng.standard_normal((N, 1, n))).astype(F32)
        rec, state = tp.walk(x, state)
        t = torch.from_numpy(x).cuda()
        m.process_dev(t.data_ptr())
        got = m.collect()
        assert tp.same(got, rec), call
        assert tp.same(m.state(), state), call
    m.close()


def test_arguments_are_checked(fmrx):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = fmrx.TruePeak(1, 2, 16)
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
    assert not m.collect()["true_peak"].any()
    m.close()
    for bad in (dict(n_channels=0), dict(audio_channels=3), dict(n_audio=0), dict(n_audio=2 ** 26 + 1), dict(limit=0.0), dict(limit=float("nan")),
                dict(limit=float("inf")), dict(limit=-1.0)):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.TruePeak(**bad)
        assert e.value.code == fmrx.EINVAL
