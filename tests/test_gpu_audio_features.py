"""The audio feature frames' kernel against the model (tests/_audio_features_model.py), bit for bit in
features, frame counts and state (any NaN equal to any NaN): random rows at the small geometry G0 over channel counts whose tiles
straddle channels and end ragged, both presets, fills that differ between channels, calls shorter than a frame, pitched and
4-byte-aligned rows, one long row, special values, the host call, a second call before collect, the results on the device as a
torch tensor, a bank of more channels than a grid's y holds, and the refusals.

The model takes its tables from the library (they are the definition); tests/test_audio_features_model_host.py checks them."""
import numpy as np
import pytest

import _audio_features_model as af

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = F32(3e38)                      # what lies between the rows and behind the last: a load past n reads infinity or NaN
G0 = af.G0
_tables = {}


def tables(fmrx, g):
    key = tuple(g[k] for k in af.FIELDS)
    if key not in _tables:
        _tables[key] = fmrx.audioFeaturesTables(g)
    return _tables[key]


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


def check(m, feat, frames, state, where=None):
    """the handle's results and state against the model's; the model's feat holds F_max(n) frames, the handle's F_max(n_audio)"""
    got, got_frames = m.collect()
    assert got.shape == (m.n_channels, m.max_frames, m.n_mels) and np.array_equal(got_frames, frames), (where, got_frames, frames)
    assert af.same(got[:, :feat.shape[1]], feat), where
    assert not got[:, feat.shape[1]:].any(), where
    for c in range(m.n_channels):
        assert not got[c, frames[c]:].view(np.uint32).any(), (where, c)          # frames the call did not complete read +0
    assert af.same(m.state(), state), where
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------
_refs = {}


def reference(fmrx, ac, n_audio):
    """37 channels at G0, three calls with the state carried -> per call (rows, feat, frames, the state after)"""
    key = (ac, n_audio)
    if key not in _refs:
        rng = np.random.default_rng(100 * ac + n_audio)
        state, out = af.fresh(37), []
        for n in (n_audio, max(1, n_audio // 3), n_audio - 1):
            x = (0.9 * rng.standard_normal((37, ac, n))).astype(F32)
            feat, frames, state = af.walk(x, state, G0, tables(fmrx, G0))
            out.append((x, feat, frames, state))
        _refs[key] = out
    return _refs[key]


@pytest.mark.parametrize("n_audio", [100, 257])
@pytest.mark.parametrize("N", [1, 5, 37])
@pytest.mark.parametrize("ac", [1, 2])
def test_1_random_rows_equal_the_model(fmrx, ac, N, n_audio):
    """F_max = 5 or 11: 16 columns straddle channels, and the last tile is ragged (N F_max is 5, 25, 185, 11, 55, 407)"""
    import torch
    m = fmrx.AudioFeatures(N, ac, n_audio, G0)
    assert m.max_frames == af.max_frames(n_audio, G0) == (n_audio - 1) // 24 + 1 and (N * m.max_frames) % 16 != 0
    total = 0
    for call, (x, feat, frames, state) in enumerate(reference(fmrx, ac, n_audio)):
        t, ptr, pitch = on_device(torch, x[:N])
        m.process_dev(ptr, pitch, x.shape[2])
        got = check(m, feat[:N], frames[:N], state[:N], call)
        assert np.isfinite(got).all()                                  # no load past n: POISON would show
        total += int(frames[0])
    assert total == (sum(x.shape[2] for x, _, _, _ in reference(fmrx, ac, n_audio)) - 64) // 24 + 1      # frames straddle the calls
    m.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def test_2_the_48_khz_preset(fmrx):
    import torch
    g = af.PRESETS[48000.0]
    p = fmrx.audioFeaturesPreset(48000.0)
    assert {k: getattr(p, k) for k in af.FIELDS} == g
    N, ac, n = 3, 2, 1920
    m = fmrx.AudioFeatures(N, ac, n)                                   # params None: the 48 kHz preset
    assert m.max_frames == 4 and m.n_mels == 80
    rng = np.random.default_rng(2)
    state = af.fresh(N)
    for call, F in enumerate((2, 4)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        feat, frames, state = af.walk(x, state, g, tables(fmrx, g))
        assert (frames == F).all()
        t, ptr, pitch = on_device(torch, x)
        m.process_dev(ptr, pitch, n)
        got = check(m, feat, frames, state, call)
        assert (got[:, :F] > 0).all()
    assert (state["fill"] == 960).all()                                # the steady state of a bank row: 960 carried, 4 frames per call
    m.close()


def test_2_the_44_1_khz_preset_on_a_mode_2_row(fmrx):
    import torch
    mp = fmrx.modeParams(2)
    assert mp.audio_Fs == 44100.0
    n = mp.block_bytes // 2 // mp.rf_decim * mp.audio_upsamp // mp.audio_decim        # the row a mode-2 bank writes per block
    assert n == 1029
    g = af.PRESETS[44100.0]
    p = fmrx.audioFeaturesPreset(mp.audio_Fs)
    assert {k: getattr(p, k) for k in af.FIELDS} == g
    N, ac = 2, 1
    m = fmrx.AudioFeatures(N, ac, n, p)
    assert m.max_frames == 3
    rng = np.random.default_rng(22)
    state, seen = af.fresh(N), []
    for call in range(3):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        feat, frames, state = af.walk(x, state, g, tables(fmrx, g))
        t, ptr, pitch = on_device(torch, x, wide=False)
        m.process_dev(ptr, pitch, n)
        check(m, feat, frames, state, call)
        seen.append(int(frames[0]))
    assert seen == [0, 3, 2]                                           # 1029, 2058, 3087 samples: 0, 3 and 5 frames of 1104 at a hop of 441
    m.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_3_reset_of_one_channel_leaves_its_neighbours_alone(fmrx):
    N, ac, n = 7, 2, 100
    rng = np.random.default_rng(3)
    t = tables(fmrx, G0)
    m = fmrx.AudioFeatures(N, ac, n, G0)
    state = af.fresh(N)
    differ = False
    for call, gone in enumerate((None, 3, None, 0, 6, None)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        feat, frames, state = af.walk(x, state, G0, t)
        got, got_frames = m.process(x)
        assert af.same(got[:, :feat.shape[1]], feat) and np.array_equal(got_frames, frames) and af.same(m.state(), state), call
        differ |= len(set(frames.tolist())) > 1
        if gone is not None:
            m.reset(gone)
            state[gone] = np.zeros((), af.STATE_DTYPE)                 # its own stream restarts; the model's other channels go on
            assert af.same(m.state(), state), call
    assert differ and len(set(state["fill"].tolist())) > 1             # frames and fills now differ between the channels
    m.reset()
    st = m.state()
    assert not st["fill"].any() and not st["carry"].any()
    m.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [1, 2])
def test_4_short_calls_pitched_rows_and_4_byte_alignment(fmrx, ac):
    import torch
    N, n_audio = 5, 100
    rng = np.random.default_rng(40 + ac)
    t = tables(fmrx, G0)
    m = fmrx.AudioFeatures(N, ac, n_audio, G0)
    state = af.fresh(N)
    for call, (n, wide) in enumerate(((7, True), (20, False), (36, True), (1, False), (63, False), (100, False), (99, True))):
        fill = int(state["fill"][0])
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        feat, frames, state = af.walk(x, state, G0, t)
        tt, ptr, pitch = on_device(torch, x, wide)                     # pitch > n, POISON behind every row
        assert pitch > n and (wide or ptr % 16 == 4)
        m.process_dev(ptr, pitch, n)
        got = check(m, feat, frames, state, call)
        assert np.isfinite(got).all()
        if fill + n < 64:
            assert not frames.any() and not got.view(np.uint32).any() and (state["fill"] == fill + n).all()      # F = 0: the state grows
    m.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_5_one_long_row(fmrx):
    """n = 2^16 + 123: 2 734 frames in 171 tiles of one channel.  The host walk is the reference here (the host tests hold it to the
    model); the same stream fed as bank-length calls gives the same frames"""
    import torch
    n = 2 ** 16 + 123
    rng = np.random.default_rng(5)
    x = (0.9 * rng.standard_normal((1, 1, n))).astype(F32)
    want, F, st = fmrx.audioFeaturesWalk(x[0], G0)
    assert F == (n - 64) // 24 + 1 == 2734 and want.shape[0] == af.max_frames(n, G0)
    m = fmrx.AudioFeatures(1, 1, n, G0)
    t, ptr, pitch = on_device(torch, x, wide=False)
    m.process_dev(ptr, pitch, n)
    got, frames = m.collect()
    assert frames[0] == F and af.same(got[0], want) and af.same(m.state()[0], st)
    m.close()
    b = fmrx.AudioFeatures(1, 1, 1920, G0)
    parts = []
    for a in range(0, n, 1920):
        feat, frames = b.process(x[:, :, a:a + 1920])
        parts.append(feat[0, :frames[0]])
    assert np.concatenate(parts).tobytes() == want[:F].tobytes() and af.same(b.state()[0], st)
    b.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [1, 2])
def test_6_special_values_across_frame_tile_and_call_boundaries_equal_the_model(fmrx, ac):
    import torch
    N, n = 6, 257                          # F_max = 11: tiles end inside channels
    rng = np.random.default_rng(60 + ac)
    t = tables(fmrx, G0)
    m = fmrx.AudioFeatures(N, ac, n, G0)
    state = af.fresh(N)
    sv = np.array([2.0, -2.0, -0.0, 1e-40, -3e-45, 1.17549435e-38, 0.0, -1e-39, 2.0, -2.0, 1e-40, -0.0], F32)
    seen_nan = seen_inf = False
    for call in range(3):
        fill = int(state["fill"][0])
        x = af.special_rows(rng, N, ac, n)
        edge = 3 * 24 - fill + 24 * 2                                  # a frame's first sample, in the row
        x[0, 0, edge - 6:edge + 6] = sv                                # across a frame edge
        x[1, ac - 1, n - 5:] = [1e-40, -2.0, -0.0, 2.0, -3e-45]        # across the call's end
        x[1, 0, :4] = [-2.0, 1e-40, -0.0, 2.0]                         # and its start
        x[2, :, :] = rng.choice(np.array([1e-40, -3e-45, 1.17549435e-38, -0.0, 0.0, -1e-39], F32), (ac, n))      # denormals and zeros alone
        x[3, ac - 1, n - 3] = np.nan                                   # a NaN in the carried samples: the next call completes its frames
        x[4, 0, 100], x[4, 0, 105] = np.inf, -np.inf                   # both signs in overlapping frames
        x[5, 0, 130] = -0.0
        feat, frames, state = af.walk(x, state, G0, t)
        tt, ptr, pitch = on_device(torch, x, wide=bool(call % 2))
        m.process_dev(ptr, pitch, n)
        check(m, feat, frames, state, call)
        F = int(frames[0])
        assert np.isfinite(feat[:3]).all() and np.isfinite(feat[5]).all() and not feat[2].any()      # the denormals' squares underflow
        if call > 0:
            seen_nan |= bool(np.isnan(feat[3, 0, 1:]).all())           # the first frame of the call holds the last call's NaN
        seen_inf |= bool((~np.isfinite(feat[4, :F, 1:])).any())
    assert seen_nan and seen_inf
    m.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_7_the_host_call_returns_the_device_calls_bytes(fmrx):
    import torch
    N, ac, n = 37, 2, 257
    x = reference(fmrx, ac, n)[0][0]
    a, b = fmrx.AudioFeatures(N, ac, n, G0), fmrx.AudioFeatures(N, ac, n, G0)
    feat_h, frames_h = a.process(x)
    t = torch.from_numpy(x).cuda()
    b.process_dev(t.data_ptr())
    feat_d, frames_d = b.collect()
    assert feat_h.tobytes() == feat_d.tobytes() and frames_h.tobytes() == frames_d.tobytes() and a.state().tobytes() == b.state().tobytes()
    assert af.same(feat_h, reference(fmrx, ac, n)[0][1])
    with pytest.raises(fmrx.FmrxError):
        a.process(np.zeros((N, ac, n + 1), F32))     # more than the handle's n_audio
    a.close()
    b.close()


def test_7_a_second_call_before_collect_replaces_the_results(fmrx):
    import torch
    N, ac, n = 5, 2, 257
    (x0, _, _, _), (x1, feat1, frames1, state1), _ = reference(fmrx, ac, n)
    m = fmrx.AudioFeatures(N, ac, n, G0)
    stream = torch.cuda.Stream()
    t0, t1 = torch.from_numpy(x0[:N]).cuda(), torch.from_numpy(np.ascontiguousarray(x1[:N])).cuda()
    torch.cuda.synchronize()
    m.process_dev(t0.data_ptr(), stream=stream.cuda_stream)
    m.process_dev(t1.data_ptr(), x1.shape[2], x1.shape[2], stream=stream.cuda_stream)
    check(m, feat1[:N], frames1[:N], state1[:N])      # the second call's results; the state advanced by both
    stream.synchronize()
    m.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_8_the_results_on_the_device_as_a_torch_tensor(fmrx):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    N, ac, n = 5, 1, 257
    x = reference(fmrx, ac, n)[0][0][:N]
    m = fmrx.AudioFeatures(N, ac, n, G0)
    t = torch.from_numpy(x).cuda()
    m.process_dev(t.data_ptr())
    feat_ptr, frames_ptr, shape = m.result_dev()
    assert shape == (N, 11, 10) and feat_ptr % 16 == 0

    class Wrapped:                                     # what a consumer hands torch: the pointer, the shape, float32
        def __init__(self, ptr, shape, typestr):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2)

    torch.cuda.synchronize()                           # the call ran on the null stream; the tensors below read after it
    feat = torch.as_tensor(Wrapped(feat_ptr, shape, "<f4"), device="cuda")
    frames = torch.as_tensor(Wrapped(frames_ptr, (N,), "<i4"), device="cuda")
    want, want_frames = m.collect()
    assert feat.dtype == torch.float32 and tuple(feat.shape) == shape
    assert feat.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(frames.cpu().numpy().astype(np.uint32), want_frames)
    logmel = torch.log10(feat[:, :int(want_frames[0])].clamp_min(1e-10))       # the logarithm is the caller's
    assert bool(torch.isfinite(logmel).all())
    m.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_9_a_bank_of_66_000_mono_channels(fmrx):
    """more channels than a grid's y or z holds: the tiles ride in x.  Every channel has a row of its own; 64 of them, the first and
    the last included, are checked against the host walk"""
    import torch
    N, n = 66000, 100
    rng = np.random.default_rng(9)
    x = (0.9 * rng.standard_normal((N, 1, n))).astype(F32)
    m = fmrx.AudioFeatures(N, 1, n, G0)
    t = torch.from_numpy(x).cuda()
    m.process_dev(t.data_ptr())
    got, frames = m.collect()
    assert (frames == 2).all() and not got[:, 2:].any()
    st = m.state()
    assert (st["fill"] == 100 - 48).all()
    pick = np.unique(np.concatenate([[0, N - 1, 65535, 65536], rng.integers(0, N, 60)]))
    for c in pick:
        want, F, ws = fmrx.audioFeaturesWalk(x[c], G0)
        assert F == 2 and af.same(got[c], want) and af.same(st[c], ws), c
    m.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_10_arguments_are_checked(fmrx):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = fmrx.AudioFeatures(1, 2, 16, G0)
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
    feat, frames = m.collect()
    assert not feat.any() and frames[0] == 0 and m.state()["fill"][0] == 16
    m.close()
    for bad in (dict(n_channels=0), dict(audio_channels=3), dict(n_audio=0), dict(n_audio=2 ** 26 + 1), dict(params=dict(G0, win=62)),
                dict(params=dict(G0, hop=65)), dict(params=dict(G0, n_bins=33)), dict(params=dict(G0, n_mels=129)),
                dict(params=dict(G0, f_hi=24001.0))):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.AudioFeatures(**{**dict(params=G0), **bad})
        assert e.value.code == fmrx.EINVAL
