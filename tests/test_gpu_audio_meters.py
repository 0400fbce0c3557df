"""The audio meters' kernel against the model (tests/_audio_meters_model.py), bit for bit (any NaN equal
to any NaN): random rows over the channel counts, lengths and both fetch paths, the special values, the decay of a float32
denormal impulse through float64 denormals, reset, the host call, the untouched input, and a second call before collect.

One reference per (audio_channels, n_audio): the model walks 130 channels at once, three calls with the state carried, and a
handle of N channels is given the first N of them -- the model's channels do not depend on each other."""
import numpy as np
import pytest

import _audio_meters_model as am

pytestmark = pytest.mark.gpu

FS = 48000.0
CHANNELS = (1, 3, 64, 65, 130)          # one lane; a part of a wave; a whole wave; a wave and a lane; two waves and a part
N_AUDIO = (1, 7, 1920, 4800, 4801, 10007)
POISON = np.float32(3e38)               # what lies between the rows: a load past n would show in peak and over
_refs = {}


def calls_of(n_audio):
    """the three calls' lengths: the handle's n_audio, then two shorter ones (n <= n_audio is allowed; no multiples of 4)"""
    return (n_audio, max(1, n_audio // 3), max(1, n_audio // 2))


def reference(ac, n_audio):
    """-> per call (rows [130][ac][n], records, bins [130][2][max_bins], the state after)"""
    key = (ac, n_audio)
    if key not in _refs:
        rng = np.random.default_rng(1000 * ac + n_audio)
        state, out = am.fresh(max(CHANNELS)), []
        for n in calls_of(n_audio):
            x = (0.7 * rng.standard_normal((max(CHANNELS), ac, n))).astype(np.float32)
            rec, bins, state = am.walk(FS, x, state, am.max_bins(FS, n_audio))
            out.append((x, rec, bins, state))
        _refs[key] = out
    return _refs[key]


def on_device(torch, x, wide):
    """rows [N][ac][n] -> (tensor, data pointer, pitch): 16-byte aligned rows in a pitch that is a multiple of 4, or the base off by
    one float and an odd pitch; POISON between the rows"""
    N, ac, n = x.shape
    pitch = (n + 3) // 4 * 4 + 4 if wide else n + 1 + n % 2
    assert pitch > n and (pitch % 4 == 0 if wide else pitch % 2 == 1)
    host = np.full(N * ac * pitch + 1, POISON, np.float32)
    off = 0 if wide else 1
    host[off:off + N * ac * pitch].reshape(N, ac, pitch)[:, :, :n] = x
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, pitch, host


def check_state(got, want, N, ac):
    assert am.same(got["z"][:, :ac], want["z"][:N, :ac]) and am.same(got["bin_acc"][:, :ac], want["bin_acc"][:N, :ac])
    assert np.array_equal(got["bin_fill"].astype(np.int64), want["bin_fill"][:N])


@pytest.mark.parametrize("n_audio", N_AUDIO)
@pytest.mark.parametrize("ac", [1, 2])
def test_1_random_rows_equal_the_model(fmrx, ac, n_audio):
    import torch
    ref = reference(ac, n_audio)
    for N in CHANNELS:
        for wide in (True, False):
            m = fmrx.AudioMeters(FS, N, ac, n_audio)
            assert m.bin_len == 4800 and m.max_bins == n_audio // 4800 + 1
            for x, rec, bins, state in ref:
                t, ptr, pitch, host = on_device(torch, x[:N], wide)
                m.process_dev(ptr, pitch, x.shape[2])
                got_rec, got_bins = m.collect()
                where = (N, wide, x.shape[2])
                assert am.same(got_rec, rec[:N]), where
                assert am.same(got_bins, bins[:N]), where
                check_state(m.state(), state, N, ac)
                assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)), where      # 6: the input is untouched
            m.close()


@pytest.mark.parametrize("ac", [1, 2])
def test_2_special_values_equal_the_model(fmrx, ac):
    import torch
    N, n = 5, 1920
    rng = np.random.default_rng(2 + ac)
    state = am.fresh(N)
    handles = {wide: fmrx.AudioMeters(FS, N, ac, n) for wide in (True, False)}
    seen_nan = False
    for call in range(3):                                   # 3 x 1920: the bin closes in the third call
        x = am.special_rows(rng, N, ac, n)
        rec, bins, state = am.walk(FS, x, state)
        for wide, m in handles.items():
            t, ptr, pitch, _ = on_device(torch, x, wide)
            m.process_dev(ptr, pitch, n)
            got_rec, got_bins = m.collect()
            assert am.same(got_rec, rec), (call, wide)
            assert am.same(got_bins, bins), (call, wide)
            check_state(m.state(), state, N, ac)
        seen_nan = seen_nan or bool(np.isnan(rec["sum_k2"][-2, 0]) and np.isinf(rec["peak"][-1, ac - 1]))
        assert rec["over"][:3, :ac].min() > 0 and np.isfinite(rec["sum_k2"][:3]).all()
    assert seen_nan and rec["bins_done"][0] == 1 and np.isnan(bins[-1, ac - 1, 0])      # poisoned until reset
    for m in handles.values():
        m.reset(N - 1)
        got_rec, _ = m.process(np.zeros((N, ac, 8), np.float32))
        assert got_rec["sum_k2"][-1, ac - 1] == 0.0 and np.isnan(got_rec["sum_k2"][-2, 0])
        m.close()


def test_3_a_denormal_impulse_decays_through_float64_denormals_with_the_models_bits(fmrx):
    """A float32 denormal impulse, then 2^17 zeros in calls of 4800: state, sums and bins keep the model's bits all the way down.
    Under round to nearest the state does not reach zero: 0.995 times a few units of the last denormal place rounds back to
    itself, so the walk ends in a fixed point a few hundred units above zero -- in the model (IEEE arithmetic, which is the
    definition) and on the device alike.  A device that flushed float64 denormals would read zero there."""
    import torch
    n, total = 4800, 1 << 17
    m = fmrx.AudioMeters(FS, 1, 1, n)
    x = np.zeros((1, 1, n), np.float32)
    x[0, 0, 0] = np.float32(1e-45)                         # the smallest float32 denormal
    assert 0 < x[0, 0, 0] < np.finfo(np.float32).tiny
    state = dict(z=[0.0] * 4, bin_acc=0.0, bin_fill=0)
    zeros = torch.zeros(n, dtype=torch.float32, device="cuda")
    first = torch.from_numpy(x.reshape(-1)).cuda()
    denormal_states, denormal_bins, states = 0, 0, []
    for call in range((total + n - 1) // n + 1):
        rec, bins, state = am.walk_scalar(FS, x[0, 0] if call == 0 else np.zeros(n, np.float32), state)
        m.process_dev((first if call == 0 else zeros).data_ptr(), n, n)
        got_rec, got_bins = m.collect()
        got = m.state()[0]
        assert got["z"][0].tobytes() == np.array(state["z"]).tobytes(), call
        assert got["bin_acc"][0] == state["bin_acc"] and got["bin_fill"] == state["bin_fill"] == 0
        assert got_rec["sum_k2"][0, 0].tobytes() == np.float64(rec["sum_k2"]).tobytes() and got_rec["sum_x"][0, 0] == rec["sum_x"], call
        assert got_bins[0, 0].tobytes() == np.array(bins).tobytes() and got_rec["bins_done"][0] == 1, call
        tiny = np.abs(np.array(state["z"][2:]))
        denormal_states += int(((tiny > 0) & (tiny < np.finfo(np.float64).tiny)).all())
        denormal_bins += int(0 < bins[0] < np.finfo(np.float64).tiny)
        states.append(state["z"])
    print(f"calls whose high-pass state ends in float64 denormals: {denormal_states}; bins that are denormal sums: {denormal_bins}; "
          f"the last state: {states[-1]}")
    assert call * n >= total and denormal_states >= 2 and denormal_bins >= 1
    assert states[-1] == states[-2] and all(0 < abs(v) < 1e-320 for v in states[-1])      # the fixed point
    m.close()


def test_4_reset_of_one_channel_leaves_its_neighbours_alone(fmrx):
    N, ac, n = 66, 2, 1920
    rng = np.random.default_rng(4)
    m = fmrx.AudioMeters(FS, N, ac, n)
    state = am.fresh(N)
    for call, gone in enumerate((1, 64, None)):
        x = (0.5 * rng.standard_normal((N, ac, n))).astype(np.float32)
        rec, bins, state = am.walk(FS, x, state)
        got_rec, got_bins = m.process(x)
        assert am.same(got_rec, rec) and am.same(got_bins, bins), call
        check_state(m.state(), state, N, ac)
        if gone is not None:
            m.reset(gone)
            for k in ("z", "bin_acc", "bin_fill"):
                state[k][gone] = 0
            check_state(m.state(), state, N, ac)
    m.reset()
    check_state(m.state(), am.fresh(N), N, ac)
    m.close()


def test_5_the_host_call_returns_the_device_calls_bytes(fmrx):
    import torch
    N, ac, n = 65, 2, 4801
    x = reference(ac, n)[0][0][:N]
    a, b = fmrx.AudioMeters(FS, N, ac, n), fmrx.AudioMeters(FS, N, ac, n)
    rec_h, bins_h = a.process(x)
    t = torch.from_numpy(x).cuda()
    b.process_dev(t.data_ptr())
    rec_d, bins_d = b.collect()
    assert rec_h.tobytes() == rec_d.tobytes() and bins_h.tobytes() == bins_d.tobytes() and a.state().tobytes() == b.state().tobytes()
    assert am.same(rec_h, reference(ac, n)[0][1][:N])
    with pytest.raises(fmrx.FmrxError):
        a.process(np.zeros((N, ac, n + 1), np.float32))     # more than the handle's n_audio
    a.close()
    b.close()


def test_6_the_input_is_untouched(fmrx):
    """(test 1 checks the same on every one of its buffers, the space between the rows included)"""
    import torch
    N, ac, n = 65, 2, 1920
    x = reference(ac, n)[0][0][:N]
    for wide in (True, False):
        m = fmrx.AudioMeters(FS, N, ac, n)
        t, ptr, pitch, host = on_device(torch, x, wide)
        m.process_dev(ptr, pitch, n)
        m.collect()
        assert np.array_equal(t.cpu().numpy().view(np.uint32), host.view(np.uint32)), wide
        m.close()


def test_7_a_second_call_before_collect_replaces_the_results(fmrx):
    import torch
    N, ac, n = 3, 2, 4800
    (x0, _, _, _), (x1, rec1, bins1, state1), _ = reference(ac, n)
    m = fmrx.AudioMeters(FS, N, ac, n)
    stream = torch.cuda.Stream()
    t0, t1 = torch.from_numpy(x0[:N]).cuda(), torch.from_numpy(np.ascontiguousarray(x1[:N])).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    m.process_dev(t1.data_ptr(), x1.shape[2], x1.shape[2], stream=stream.cuda_stream)
    got_rec, got_bins = m.collect()
    assert am.same(got_rec, rec1[:N]) and am.same(got_bins, bins1[:N])      # the second call's results; the state advanced by both
    check_state(m.state(), state1, N, ac)
    stream.synchronize()
    m.close()


def test_8_the_host_call_runs_behind_a_device_call_on_another_stream(fmrx):
    """process_dev on a non-blocking stream, then at once the host call, which runs on the null stream: its results are those of
    the two calls in that order.  (A race need not lose: this pins the sequence's result; that the host call waits for the
    handle's last call first is read in meter_stage.hpp's read_host.)"""
    import torch
    N, ac = 3, 2
    n = am.bin_len(FS) + 3                                 # a bin closes within each call
    assert n == 4803
    rng = np.random.default_rng(8)
    x0, x1 = ((0.7 * rng.standard_normal((N, ac, n))).astype(np.float32) for _ in range(2))
    _, _, state0 = am.walk(FS, x0, am.fresh(N), am.max_bins(FS, n))
    rec1, bins1, state1 = am.walk(FS, x1, state0, am.max_bins(FS, n))
    m = fmrx.AudioMeters(FS, N, ac, n)
    stream = torch.cuda.Stream()
    t0 = torch.from_numpy(x0).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    got_rec, got_bins = m.process(x1)
    assert am.same(got_rec, rec1) and am.same(got_bins, bins1) and (got_rec["bins_done"] == 1).all()
    check_state(m.state(), state1, N, ac)
    stream.synchronize()
    m.close()


def test_arguments_are_checked(fmrx):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = fmrx.AudioMeters(FS, 1, 2, 16)
    for args in ((t.data_ptr(), 16, 17), (t.data_ptr(), 8, 16), (t.data_ptr(), 16, 0), (t.data_ptr() + 2, 16, 16), (None, 16, 16)):
        with pytest.raises(fmrx.FmrxError) as e:
            m.process_dev(*args)
        assert e.value.code == fmrx.EINVAL
    with pytest.raises(fmrx.FmrxError):
        m.collect()                                        # no call yet
    with pytest.raises(fmrx.FmrxError):
        m.reset(1)
    m.close()
    for bad in (dict(audio_Fs=1e6), dict(n_channels=0), dict(audio_channels=3), dict(n_audio=0)):
        with pytest.raises(fmrx.FmrxError):
            fmrx.AudioMeters(**bad)
