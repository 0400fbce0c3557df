"""The audio rate converter's kernel against the model (tests/_audio_resample_model.py), bit for bit in the
float rows, the PCM, the counts and the state (any NaN equal to any NaN): random rows over mono and stereo, mix and per row and four
geometries, short calls on pitched and 4-byte-aligned rows, several calls against one, the reset of one channel, one long row over
many tiles, special values, the host call, a second call before collect, the results on the device as a torch tensor, a bank of more
channels than a grid's y holds, and the refusals.

The model takes its taps from the library (they are the definition); tests/test_audio_resample_model_host.py checks them."""
import numpy as np
import pytest

import _audio_resample_model as ar

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = F32(3e38)                      # what lies between the rows and behind the last: a load past n reads infinity or NaN
GEOMETRIES = {"1/3": ar.preset(48000, 16000), "147/160": ar.preset(48000, 44100), "160/441": ar.preset(44100, 16000), "3/7": ar.G_SMALL}
SHAPES = [(1, 1), (1, 0), (2, 1), (2, 0)]          # (audio_channels, mix)
TILE = 1024                                        # outputs of a workgroup at these geometries
_taps = {}


def taps(fmrx, g):
    key = tuple(g[k] for k in ar.FIELDS if k != "mix")
    if key not in _taps:
        _taps[key] = fmrx.audioResampleTaps(g)
    return _taps[key]


def on_device(torch, x, wide=True):
    """rows [N][ac][n] -> (tensor, data pointer, pitch): 16-byte aligned rows in a pitch that is a multiple of 4, or the base off by
    one float and an odd pitch; POISON between the rows and behind the last"""
    N, ac, n = x.shape
    pitch = (n + 3) // 4 * 4 + 4 if wide else n + 1 + n % 2
    host = np.full(N * ac * pitch + 1 + 16, POISON, F32)
    off = 0 if wide else 1
    host[off:off + N * ac * pitch].reshape(N, ac, pitch)[:, :, :n] = x
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, pitch


def check(m, oracle, want, counts, state, wrap=True, where=None):
    """the handle's results and state against the model's; the model's rows hold max_out(n) entries, the handle's max_out(n_audio)"""
    got = m.collect()
    full = np.zeros(m.shape, F32)
    full[:, :, :want.shape[2]] = want
    assert np.array_equal(got["counts"], counts), (where, got["counts"], counts)
    if m.want_f32:
        assert got["audio"].shape == m.shape and ar.same(got["audio"], full), where
        for c in range(m.n_channels):
            assert not got["audio"][c, :, counts[c]:].view(np.uint32).any(), (where, c)      # beyond the count: +0
    else:
        assert got["audio"] is None
    if m.want_pcm:
        assert np.array_equal(got["pcm16"], oracle.pcm16(full.reshape(-1), wrap).reshape(m.shape)), where
    else:
        assert got["pcm16"] is None
    assert ar.same(m.state(), state), where
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
_refs = {}


def reference(fmrx, ac, mix, name, N=5, n_audio=1920):
    """N channels, three calls with the state carried -> per call (rows, out, counts, the state after)"""
    key = (ac, mix, name, N, n_audio)
    if key not in _refs:
        g = dict(GEOMETRIES[name], mix=mix)
        rng = np.random.default_rng(1000 * ac + 100 * mix + len(name) + n_audio)
        state, calls = ar.fresh(N), []
        for n in (n_audio, n_audio // 3, n_audio - 1):
            x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
            out, counts, state = ar.walk(x, state, g, taps(fmrx, g))
            calls.append((x, out, counts, state))
        _refs[key] = calls
    return _refs[key]


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac,mix", SHAPES)
def test_1_random_rows_equal_the_model(fmrx, oracle, ac, mix, name):
    import torch
    g = dict(GEOMETRIES[name], mix=mix)
    N, n_audio = 5, 1920
    m = fmrx.AudioResample(N, ac, n_audio, g, want_f32=True, want_pcm=True)
    assert m.max_out == ar.max_out(n_audio, g) and m.rows == ar.rows_of(g, ac) and m.latency == ar.latency(g)
    total = 0
    for call, (x, out, counts, state) in enumerate(reference(fmrx, ac, mix, name)):
        t, ptr, pitch = on_device(torch, x)
        m.process_dev(ptr, pitch, x.shape[2], wrap=call != 1)
        got = check(m, oracle, out, counts, state, call != 1, call)
        assert np.isfinite(got["audio"]).all()                         # no load past n: POISON would show
        total += int(counts[0])
    assert total == ar.outputs_of(1920 + 640 + 1919, g, 0)             # the calls continue one stream
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac,mix", [(1, 1), (2, 1), (2, 0)])
def test_2_short_calls_pitched_rows_and_4_byte_alignment(fmrx, oracle, ac, mix, name):
    import torch
    g = dict(GEOMETRIES[name], mix=mix)
    T, N, n_audio = g["taps"], 5, 1920
    rng = np.random.default_rng(20 + ac + mix + len(name))
    h = taps(fmrx, g)
    m = fmrx.AudioResample(N, ac, n_audio, g, want_f32=True, want_pcm=True)
    state = ar.fresh(N)
    for call, (n, wide) in enumerate(((1, True), (3, False), (T - 2, True), (T - 1, False), (T, False), (1919, False), (1, False), (1919, True))):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        out, counts, state = ar.walk(x, state, g, h)
        tt, ptr, pitch = on_device(torch, x, wide)                     # pitch > n, POISON behind every row
        assert pitch > n and (wide or ptr % 16 == 4)
        m.process_dev(ptr, pitch, n, wrap=False)
        got = check(m, oracle, out, counts, state, False, (call, n))
        assert np.isfinite(got["audio"]).all() and np.abs(got["audio"]).max() < 10.0
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_3_several_calls_equal_one(fmrx, name):
    import torch
    g = dict(GEOMETRIES[name], mix=1)
    N, ac, n = 3, 2, 1920
    rng = np.random.default_rng(30 + len(name))
    x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
    one, parts = fmrx.AudioResample(N, ac, n, g), fmrx.AudioResample(N, ac, n, g)
    t = torch.from_numpy(x).cuda()
    one.process_dev(t.data_ptr())
    whole = one.collect()
    pieces, a = [], 0
    for k in (700, 13, 1207):
        tt, ptr, pitch = on_device(torch, x[:, :, a:a + k], wide=False)
        parts.process_dev(ptr, pitch, k)
        got = parts.collect()
        assert len(set(got["counts"].tolist())) == 1
        pieces.append(got["audio"][:, :, :got["counts"][0]])
        a += k
    M = int(whole["counts"][0])
    assert a == n and M == ar.max_out(n, g)
    assert np.concatenate(pieces, axis=2).tobytes() == whole["audio"][:, :, :M].tobytes()
    assert one.state().tobytes() == parts.state().tobytes()
    one.close()
    parts.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["147/160", "3/7"])
def test_4_reset_of_one_channel_leaves_its_neighbours_alone(fmrx, name):
    g = dict(GEOMETRIES[name], mix=0)
    N, ac, n = 7, 2, 101
    rng = np.random.default_rng(4)
    h = taps(fmrx, g)
    m = fmrx.AudioResample(N, ac, n, g)
    state = ar.fresh(N)
    for call, gone in enumerate((None, 3, None, 0, 6, None)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        out, counts, state = ar.walk(x, state, g, h)
        got = m.process(x)
        assert ar.same(got["audio"][:, :, :out.shape[2]], out) and np.array_equal(got["counts"], counts) and ar.same(m.state(), state), call
        if gone is not None:
            m.reset(gone)
            state[gone] = np.zeros((), ar.STATE_DTYPE)                 # its own stream restarts; the model's other channels go on
            assert ar.same(m.state(), state), call
    assert len(set(state["pos"].tolist())) > 1                         # the positions now differ between the channels
    m.reset()
    st = m.state()
    assert not st["pos"].any() and not st["carry"].any()
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_5_one_long_row(fmrx, oracle, name):
    """70 000 samples: 23 to 63 tiles of 1 024 outputs.  The host walk is the reference here (the host tests hold it to the model)"""
    import torch
    g = GEOMETRIES[name]
    n = 70000
    rng = np.random.default_rng(5)
    x = (0.9 * rng.standard_normal((1, 1, n))).astype(F32)
    want, M, st = fmrx.audioResampleWalk(x[0], g)
    assert M == ar.max_out(n, g) >= 3 * TILE
    m = fmrx.AudioResample(1, 1, n, g, want_f32=True, want_pcm=True)
    t, ptr, pitch = on_device(torch, x, wide=name != "1/3")
    m.process_dev(ptr, pitch, n)
    got = m.collect()
    assert got["counts"][0] == M and ar.same(m.state()[0], st)
    bad = np.flatnonzero(got["audio"][0, 0].view(np.uint32) != want[0].view(np.uint32))
    assert bad.size == 0, (bad[:8], bad[:8] // TILE)
    assert np.array_equal(got["pcm16"][0, 0], oracle.pcm16(want[0], True))
    m.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac,mix", [(1, 1), (2, 1), (2, 0)])
def test_6_special_values_across_window_tile_and_call_boundaries_equal_the_model(fmrx, oracle, ac, mix, name):
    import torch
    g = dict(GEOMETRIES[name], mix=mix)
    U, D, T = g["up"], g["down"], g["taps"]
    N = 7
    n = -(-(TILE + 90) * D // U)                                       # a second tile of some 90 outputs
    rng = np.random.default_rng(60 + ac + mix + len(name))
    h = taps(fmrx, g)
    m = fmrx.AudioResample(N, ac, n, g, want_f32=True, want_pcm=True)
    state = ar.fresh(N)
    edge = TILE * D // U                                               # the newest input of the second tile's first output, at pos 0
    for call in range(3):
        x = ar.special_rows(rng, N, ac, n, T)
        x[0, ac - 1, edge - T // 2] = np.nan                           # in windows on both sides of the tile boundary
        x[1, 0, edge - T + 1], x[1, 0, edge] = np.inf, -np.inf         # the first tile's last windows and the second's first
        pos = int(state["pos"][0])
        out, counts, state = ar.walk(x, state, g, h)
        tt, ptr, pitch = on_device(torch, x, wide=bool(call % 2))
        m.process_dev(ptr, pitch, n, wrap=bool(call % 2))
        check(m, oracle, out, counts, state, bool(call % 2), call)
        # a NaN reaches exactly the outputs whose window holds it
        if mix or ac == 1:
            others = [s for s in range(n) if np.isnan(x[0, :, s]).any() or np.isinf(x[0, :, s]).any()]
            q = np.arange(counts[0])
            i = (pos + q * D) // U
            holds = np.zeros(len(q), bool)
            for s in others:
                holds |= (i >= s) & (i - s < T)
            assert holds[TILE - 1] and holds[TILE]
            assert not np.isfinite(out[0, 0, :counts[0]][holds]).any() and np.isfinite(out[0, 0, :counts[0]][~holds]).all()
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_7_the_host_call_returns_the_device_calls_bytes(fmrx):
    import torch
    N, ac, mix, name, n = 5, 2, 1, "160/441", 1920
    g = dict(GEOMETRIES[name], mix=mix)
    x, out, counts, _ = reference(fmrx, ac, mix, name)[0]
    a, b = fmrx.AudioResample(N, ac, n, g, True, True), fmrx.AudioResample(N, ac, n, g, True, True)
    host = a.process(x)
    t = torch.from_numpy(x).cuda()
    b.process_dev(t.data_ptr())
    dev = b.collect()
    for k in ("audio", "pcm16", "counts"):
        assert host[k].tobytes() == dev[k].tobytes(), k
    assert a.state().tobytes() == b.state().tobytes() and ar.same(host["audio"][:, :, :out.shape[2]], out)
    with pytest.raises(fmrx.FmrxError):
        a.process(np.zeros((N, ac, n + 1), F32))     # more than the handle's n_audio
    a.close()
    b.close()
    c = fmrx.AudioResample(N, ac, n, g, want_f32=False, want_pcm=True)     # PCM alone
    only = c.process(x)
    assert only["audio"] is None and only["pcm16"].tobytes() == host["pcm16"].tobytes()
    c.close()


def test_7_a_second_call_before_collect_replaces_the_results(fmrx, oracle):
    import torch
    N, ac, mix, name, n = 5, 2, 0, "147/160", 1920
    g = dict(GEOMETRIES[name], mix=mix)
    (x0, _, _, _), (x1, out1, counts1, state1), _ = reference(fmrx, ac, mix, name)
    m = fmrx.AudioResample(N, ac, n, g, True, True)
    stream = torch.cuda.Stream()
    t0, t1 = torch.from_numpy(x0).cuda(), torch.from_numpy(np.ascontiguousarray(x1)).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    m.process_dev(t1.data_ptr(), x1.shape[2], x1.shape[2], stream=stream.cuda_stream)
    check(m, oracle, out1, counts1, state1)           # the second call's results, zeros where the first's were longer; the state advanced by both
    stream.synchronize()
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_8_the_results_on_the_device_as_torch_tensors(fmrx):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    N, ac, mix, name, n = 5, 2, 0, "1/3", 1920
    g = dict(GEOMETRIES[name], mix=mix)
    x = reference(fmrx, ac, mix, name)[0][0]
    m = fmrx.AudioResample(N, ac, n, g, True, True)
    t = torch.from_numpy(x).cuda()
    m.process_dev(t.data_ptr())
    f32_ptr, pcm_ptr, counts_ptr, shape = m.result_dev()
    assert shape == (N, 2, 640) and f32_ptr % 16 == 0 and pcm_ptr % 16 == 0

    class Wrapped:                                     # what a consumer hands torch: the pointer, the shape, the type
        def __init__(self, ptr, shape, typestr):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2)

    torch.cuda.synchronize()                           # the call ran on the null stream; the tensors below read after it
    audio = torch.as_tensor(Wrapped(f32_ptr, shape, "<f4"), device="cuda")
    pcm = torch.as_tensor(Wrapped(pcm_ptr, shape, "<i2"), device="cuda")
    counts = torch.as_tensor(Wrapped(counts_ptr, (N,), "<i4"), device="cuda")
    want = m.collect()
    assert audio.dtype == torch.float32 and pcm.dtype == torch.int16 and tuple(audio.shape) == tuple(pcm.shape) == shape
    assert audio.cpu().numpy().tobytes() == want["audio"].tobytes() and pcm.cpu().numpy().tobytes() == want["pcm16"].tobytes()
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), want["counts"]) and (want["counts"] == 640).all()
    assert bool(torch.isfinite(audio.square().mean(dim=2)).all())
    m.close()
    only = fmrx.AudioResample(N, ac, n, g, want_f32=True, want_pcm=False)
    assert only.result_dev()[1] is None
    only.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_9_a_bank_of_66_000_mono_channels(fmrx):
    """more channels than a grid's y or z holds: the channel rides in x.  Every channel has a row of its own; 64 of them, the first and
    the last included, are checked against the host walk"""
    import torch
    g = ar.geometry(2, 3, 8)
    N, n = 66000, 64
    rng = np.random.default_rng(9)
    x = (0.9 * rng.standard_normal((N, 1, n))).astype(F32)
    m = fmrx.AudioResample(N, 1, n, g)
    t = torch.from_numpy(x).cuda()
    m.process_dev(t.data_ptr())
    got = m.collect()
    assert m.max_out == 43 and (got["counts"] == 43).all()
    st = m.state()
    assert (st["pos"] == 43 * 3 - 64 * 2).all()
    pick = np.unique(np.concatenate([[0, N - 1, 65535, 65536], rng.integers(0, N, 60)]))
    for c in pick:
        want, M, ws = fmrx.audioResampleWalk(x[c], g)
        assert M == 43 and ar.same(got["audio"][c], want) and ar.same(st[c], ws), c
    m.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_10_arguments_are_checked(fmrx):
    import torch
    G = ar.G_SMALL
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = fmrx.AudioResample(1, 2, 16, G)
    for args in ((t.data_ptr(), 16, 17), (t.data_ptr(), 8, 16), (t.data_ptr(), 16, 0), (t.data_ptr() + 2, 16, 16), (None, 16, 16)):
        with pytest.raises(fmrx.FmrxError) as e:
            m.process_dev(*args)
        assert e.value.code == fmrx.EINVAL
    with pytest.raises(fmrx.FmrxError) as e:
        m._call("process_dev", t.data_ptr(), 16, 16, 2, None)              # no such PCM policy
    assert e.value.code == fmrx.EINVAL
    with pytest.raises(fmrx.FmrxError):
        m.collect()                                        # no call yet: nothing was launched
    assert not m.state()["pos"].any()
    with pytest.raises(fmrx.FmrxError):
        m.reset(1)
    with pytest.raises(fmrx.FmrxError):
        m.process(np.zeros((1, 2, 17), F32))
    m.process_dev(t.data_ptr(), 16, 16)                    # and what is accepted still runs
    got = m.collect()
    assert not got["audio"].any() and got["pcm16"] is None and got["counts"][0] == 7 and m.state()["pos"][0] == 7 * 7 - 16 * 3
    pcm = np.zeros(m.shape, np.int16)
    with pytest.raises(fmrx.FmrxError):
        m._call("collect", None, pcm.ctypes.data, got["counts"].ctypes.data)      # a result the handle does not keep
    m.close()
    for bad in (dict(n_channels=0), dict(audio_channels=3), dict(n_audio=0), dict(n_audio=2 ** 26 + 1), dict(want_f32=False, want_pcm=False),
                dict(params=dict(G, up=14)), dict(params=dict(G, taps=10)), dict(params=dict(G, down=1025)), dict(params=dict(G, mix=2)),
                dict(params=dict(G, cutoff=0.0)), dict(params=dict(G, beta=21.0)), dict(params=ar.geometry(160, 1, 8), n_audio=2 ** 26)):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.AudioResample(**{**dict(params=G), **bad})
        assert e.value.code == fmrx.EINVAL
