"""The audio feature frames without a GPU (include/fmrx.h: fmrx_audio_features_*): the host walk against
the model bit for bit, that the frames do not depend on how a stream is cut into calls, the tables against a numpy float64
restatement, the model against a float64 FFT and filterbank, special values, the refusals and the exported symbols."""
import re

import numpy as np
import pytest

import _audio_features_model as af

F32, F64 = np.float32, np.float64
G0 = af.G0
GEOMETRIES = {"G0": G0, "48 kHz": af.PRESETS[48000.0], "44.1 kHz": af.PRESETS[44100.0],
              "hop = win": dict(win=16, hop=16, n_bins=8, n_mels=3, f_lo=100.0, f_hi=4000.0, audio_Fs=8000.0),
              "hop = 1": dict(win=36, hop=1, n_bins=18, n_mels=128, f_lo=0.0, f_hi=16000.0, audio_Fs=32000.0)}


def host_walk(fmrx, rows, states, g):
    """fmrx_audio_features_walk channel by channel, in the model's shapes; states is replaced"""
    N, n = rows.shape[0], rows.shape[2]
    feat, frames = np.zeros((N, af.max_frames(n, g), g["n_mels"]), F32), np.zeros(N, np.uint32)
    for c in range(N):
        feat[c], frames[c], states[c] = fmrx.audioFeaturesWalk(rows[c], g, states[c])
    return feat, frames


# ---- the host walk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac", [1, 2])
def test_1_the_host_walk_equals_the_model_bit_for_bit(fmrx, ac, name):
    g = GEOMETRIES[name]
    assert fmrx.AUDIO_FEATURES_STATE_DTYPE == af.STATE_DTYPE and af.good(g)
    t = fmrx.audioFeaturesTables(g)
    N = 3
    rng = np.random.default_rng(10 * ac + g["win"])
    model, states = af.fresh(N), af.fresh(N)
    win, hop = g["win"], g["hop"]
    T, done = 0, 0
    for call, n in enumerate((win - 1, 1, hop, win + hop + 3, 7)):           # a few frames each; the chains are slow in numpy
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        want, want_frames, model = af.walk(x, model, g, t)
        got, frames = host_walk(fmrx, x, states, g)
        assert af.same(got, want) and np.array_equal(frames, want_frames), (call, n)
        assert af.same(states, model), (call, n)
        T += n
        F = af.frames_of(T - done * hop, g)
        done += F
        assert (frames == F).all() and (states["fill"] == T - done * hop).all() and (states["fill"] < win).all()
        assert not got[:, F:].any() and not states["carry"][:, T - done * hop:].any()
        assert np.isfinite(got).all()
    assert done == af.frames_of(T, g) >= 2


def test_1_presets_max_frames_and_dtype(fmrx):
    for Fs, g in af.PRESETS.items():
        p = fmrx.audioFeaturesPreset(Fs)
        assert {k: getattr(p, k) for k in af.FIELDS} == g and af.good(g)
    assert af.PRESETS[48000.0]["audio_Fs"] / af.PRESETS[48000.0]["win"] == 40.0           # bin k sits at 40 k Hz
    for Fs in (32000.0, 0.0, 96000.0, float("nan")):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.audioFeaturesPreset(Fs)
        assert e.value.code == fmrx.EINVAL
    for g, n, want in ((af.PRESETS[48000.0], 1920, 4), (af.PRESETS[48000.0], 1, 1), (af.PRESETS[48000.0], 481, 2), (G0, 2 ** 16 + 123, 2736),
                       (af.PRESETS[44100.0], 1029, 3)):
        assert fmrx.audioFeaturesMaxFrames(g, n) == af.max_frames(n, g) == want
        for fill in range(0, g["win"], 7):                                   # no fill completes more
            assert af.frames_of(fill + n, g) <= want
        assert af.frames_of(g["win"] - 1 + n, g) == want
    assert fmrx.audioFeaturesMaxFrames(G0, 0) == 0 and fmrx.audioFeaturesMaxFrames(dict(G0, win=62), 100) == 0


# ---- cutting the stream -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [1, 2])
def test_2_the_frames_do_not_depend_on_the_cut(fmrx, ac):
    g = G0
    win, hop = g["win"], g["hop"]
    rng = np.random.default_rng(20 + ac)
    total = 20 * win + 5
    x = af.special_rows(rng, 1, ac, total)[0]
    whole, F, st = fmrx.audioFeaturesWalk(x, g)
    assert F == af.frames_of(total, g) and st["fill"] == total - F * hop < win
    want = whole[:F].tobytes()
    model, _, _ = af.walk(x[None], af.fresh(1), g, fmrx.audioFeaturesTables(g))
    assert af.same(model[0], whole)
    cuts = {"1": lambda: 1, "hop - 1": lambda: hop - 1, "hop": lambda: hop, "win - 1": lambda: win - 1, "win + 1": lambda: win + 1,
            "random": lambda: int(rng.integers(1, 3 * win))}
    for name, length in cuts.items():
        state, at, parts, fill = None, 0, [], 0
        while at < total:
            n = min(length(), total - at)
            feat, frames, state = fmrx.audioFeaturesWalk(x[:, at:at + n], g, state)
            T = fill + n
            assert frames == af.frames_of(T, g) and feat.shape[0] == af.max_frames(n, g) and not feat[frames:].any(), (name, at)
            fill = T - frames * hop
            assert state["fill"] == fill < win, (name, at)
            parts.append(feat[:frames])
            at += n
        assert np.concatenate(parts).tobytes() == want, name
        assert af.same(state, st), name


# ---- the tables ---------------------------------------------------------------------------------------------------------
def ulps(a, b):
    """the distance of float32 arrays of one sign in units of the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_3_the_tables_against_a_float64_restatement(fmrx, name):
    g = GEOMETRIES[name]
    win, n_bins, n_mels = g["win"], g["n_bins"], g["n_mels"]
    t, f = fmrx.audioFeaturesTables(g), af.formula(g)
    w, c, mel_w, lo, hi = (t[k] for k in ("window", "cosine", "mel_w", "mel_lo", "mel_hi"))
    assert w.shape == c.shape == (win,) and mel_w.shape == (n_mels, n_bins) and lo.shape == hi.shape == (n_mels,)
    # structural zeros and symmetries, exactly
    zero = np.zeros(1, F32).view(np.uint32)[0]
    assert w.view(np.uint32)[0] == zero and c.view(np.uint32)[win // 4] == zero and c.view(np.uint32)[3 * win // 4] == zero
    assert c[0] == 1.0 and c[win // 2] == -1.0 and w[win // 2] == 1.0
    m = np.arange(1, win)
    assert np.array_equal(c[win - m], c[m]) and np.array_equal(w[win - m], w[m])
    q = np.arange(0, win // 2 + 1)
    assert np.array_equal(c[win // 2 - q].view(np.uint32) & 0x7fffffff, c[q].view(np.uint32) & 0x7fffffff) and np.array_equal(c[win // 2 - q], -c[q])
    assert (mel_w >= 0).all() and np.isfinite(mel_w).all()
    # within one ulp of the float64 formulas rounded once
    differing = {}
    for k in ("window", "cosine", "mel_w"):
        d = ulps(t[k], f[k])
        differing[k] = int((d != 0).sum())
        assert d.max() <= 1, (k, int(d.max()))
    direct = np.cos(2.0 * np.pi * np.arange(win, dtype=F64) / win).astype(F32)          # no symmetry: differs at the structural zeros
    away = np.setdiff1d(np.arange(win), [win // 4, 3 * win // 4])
    assert ulps(np.abs(c[away]), np.abs(direct[away])).max() <= 1
    print(f"{name}: entries that differ from the numpy restatement: {differing}")
    # lo / hi delimit exactly the positive weights
    for b in range(n_mels):
        pos = np.flatnonzero(mel_w[b] > 0)
        if len(pos):
            assert lo[b] == pos[0] and hi[b] == pos[-1] + 1 and len(pos) == hi[b] - lo[b], b
        else:
            assert lo[b] == hi[b] == 0, b
    assert np.array_equal(lo, f["mel_lo"]) and np.array_equal(hi, f["mel_hi"])
    # a triangle's weights at its bins are the Slaney ones: the peak below 2 / (f[b+2] - f[b])
    pts = af.mel_points(g)
    assert (mel_w.max(axis=1) <= (2.0 / (pts[2:] - pts[:-2])) * (1 + 1e-6)).all()
    assert abs(pts[0] - g["f_lo"]) <= 1e-9 * max(1.0, g["f_lo"]) and abs(pts[-1] - g["f_hi"]) <= 1e-9 * g["f_hi"] and (np.diff(pts) > 0).all()


def test_3_an_empty_filter_reads_plus_zero(fmrx):
    """G0's bins are 750 Hz apart and its first filter spans 0 .. 692 Hz with a zero weight at bin 0: no bin"""
    t = fmrx.audioFeaturesTables(G0)
    pts = af.mel_points(G0)
    assert pts[0] == 0.0 and pts[2] < 750.0
    assert t["mel_lo"][0] == t["mel_hi"][0] == 0 and not t["mel_w"][0].any() and (t["mel_hi"][1:] > t["mel_lo"][1:]).all()
    x = (0.9 * np.random.default_rng(33).standard_normal((1, 64))).astype(F32)
    feat, F, _ = fmrx.audioFeaturesWalk(x, G0)
    assert F == 1 and feat.view(np.uint32)[0, 0] == 0 and (feat[0, 1:] > 0).all()
    x[0, 5] = np.nan                                   # and not a NaN either: the chain has no step
    feat, F, _ = fmrx.audioFeaturesWalk(x, G0)
    assert feat.view(np.uint32)[0, 0] == 0 and np.isnan(feat[0, 1:]).all()


def test_3_the_slaney_scale():
    assert af.hz_to_mel(1000.0) == 15.0 and af.hz_to_mel(200.0 / 3.0) == 1.0 and abs(af.hz_to_mel(6400.0) - 42.0) < 1e-12
    f = np.array([0.0, 10.0, 999.0, 1000.0, 1001.0, 8000.0, 24000.0])
    assert np.allclose(af.mel_to_hz(af.hz_to_mel(f)), f, rtol=1e-13, atol=1e-13)


# ---- against float64 ----------------------------------------------------------------------------------------------------
def features64(frames, g) -> np.ndarray:
    """np.fft.rfft of the float64 windowed frames and a float64 filterbank"""
    win = g["win"]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=F64) / win)
    p = (np.abs(np.fft.rfft(np.asarray(frames, F32).astype(F64) * w, axis=-1)) ** 2)[..., :g["n_bins"]]
    return p @ af.filterbank64(g).T


# The cap: the model's own worst deviation from float64, relative to the frame's largest feature, as measured by this test on
# noise and on noise with a tone (G0 3.4e-7, 48 kHz 1.4e-6, 44.1 kHz 1.6e-6), times a margin of 4
CAP = {"G0": 1.4e-6, "48 kHz": 5.6e-6, "44.1 kHz": 6.4e-6}


@pytest.mark.parametrize("name", list(CAP))
def test_4_the_model_against_a_float64_fft_and_filterbank(fmrx, name):
    g = GEOMETRIES[name]
    t = fmrx.audioFeaturesTables(g)
    win = g["win"]
    worst = 0.0
    for seed in range(3):
        rng = np.random.default_rng(40 + seed)
        x = 0.5 * rng.standard_normal((4, win))
        x[2:] += 1.5 * np.sin(2.0 * np.pi * (3.3 + 5.0 * seed) * np.arange(win) / win + seed)
        x = x.astype(F32)
        got, want = af.frame_features(x, g, t).astype(F64), features64(x, g)
        worst = max(worst, float((np.abs(got - want).max(axis=1) / want.max(axis=1)).max()))
    print(f"{name}: worst deviation {worst:.2e} of the frame's largest feature (cap {CAP[name]:.1e})")
    assert worst <= CAP[name]


@pytest.mark.parametrize("Fs", [48000.0, 44100.0])
def test_4_a_full_scale_sine_at_1_khz_peaks_in_its_band(fmrx, Fs):
    g = af.PRESETS[Fs]
    n = g["win"] + 2 * g["hop"]
    x = (2.0 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / Fs + 0.3)).astype(F32)
    feat, F, _ = fmrx.audioFeaturesWalk(x, g)
    assert F == 3
    pts = af.mel_points(g)
    b = int(np.argmin(np.abs(pts[1:-1] - 1000.0)))                      # the filter whose centre lies nearest; it contains 1 kHz
    assert pts[b] <= 1000.0 < pts[b + 2]
    assert (feat[:F].argmax(axis=1) == b).all(), (feat[:F].argmax(axis=1), b)
    want = features64(x[:g["win"]][None], g)[0]
    assert abs(feat[0, b] / want[b] - 1.0) < 1e-5


# ---- special values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [1, 2])
def test_5_special_values_at_frame_and_call_boundaries_equal_the_model(fmrx, ac):
    g = G0
    t = fmrx.audioFeaturesTables(g)
    N, n = 6, 150
    rng = np.random.default_rng(50 + ac)
    model, states = af.fresh(N), af.fresh(N)
    seen_nan = seen_inf = False
    for call in range(4):
        fill = int(model["fill"][0])
        x = af.special_rows(rng, N, ac, n)
        edge = 4 * 24 - fill                                           # a frame's first sample, in the row
        x[0, 0, edge - 4:edge + 4] = [2.0, -0.0, 1e-40, -3e-45, -2.0, 0.0, -1e-39, 1.17549435e-38]
        x[1, ac - 1, n - 3:] = [np.nan, -0.0, 1e-40]                   # a NaN that the call carries over
        x[2, 0, 0], x[2, ac - 1, n - 1] = np.inf, -np.inf              # at the call's two ends
        x[3, :, :] = rng.choice(np.array([1e-40, -3e-45, 1.17549435e-38, -0.0, 0.0], F32), (ac, n))
        x[4, 0, edge], x[4, 0, edge + 16] = np.inf, np.inf             # an infinity at w[0] = 0 and one at C[16] = 0 of that frame
        x[5, :, :] = F32(-0.0)
        want, want_frames, model = af.walk(x, model, g, t)
        got, frames = host_walk(fmrx, x, states, g)
        assert np.array_equal(np.isnan(got), np.isnan(want)), call                     # NaNs by position
        assert af.same(got, want) and np.array_equal(frames, want_frames) and af.same(states, model), call
        F = int(frames[0])
        assert not got[3].any() and not got[5].view(np.uint32).any() and np.isfinite(got[0]).all()
        seen_nan |= bool(call > 0 and np.isnan(got[1, 0, 1:]).all())
        seen_inf |= bool(np.isnan(got[4, :F, 1:]).any() and not np.isfinite(got[2, 0, 1:]).any())
    assert seen_nan and seen_inf


def test_5_denormal_windowed_samples_and_products_are_kept(fmrx):
    g = G0
    t = fmrx.audioFeaturesTables(g)
    x = np.zeros((1, 1, 64), F32)
    x[0, 0, 30], x[0, 0, 7] = F32(1e-19), F32(1e-40)   # 1e-19 squares into the denormal range; 1e-40 w[7] is itself denormal
    feat, F, _ = fmrx.audioFeaturesWalk(x[0], g)
    want, _, _ = af.walk(x, af.fresh(1), g, t)
    assert F == 1 and af.same(feat, want[0])
    p = af.bin_powers(x[0, 0], g, t)
    assert ((p > 0) & (p < np.finfo(F32).tiny)).sum() >= 20 and (feat[0, 1:] > 0).all() and feat.max() < 1e-38


# ---- the interface ------------------------------------------------------------------------------------------------------
BAD = (dict(win=12), dict(win=1284), dict(win=62), dict(win=0), dict(hop=0), dict(hop=65), dict(n_bins=0), dict(n_bins=33), dict(n_mels=0),
       dict(n_mels=129), dict(f_lo=-1.0), dict(f_lo=18000.0), dict(f_lo=19000.0), dict(f_hi=24000.5), dict(f_hi=float("nan")),
       dict(f_lo=float("nan")), dict(audio_Fs=float("inf")), dict(audio_Fs=float("nan")), dict(f_hi=float("inf")),
       dict(win=1280, n_bins=257, hop=1))
GOOD = (dict(), dict(win=16, hop=16, n_bins=8), dict(win=1280, hop=1, n_bins=256, n_mels=128), dict(f_hi=24000.0), dict(hop=64), dict(n_bins=32),
        dict(n_bins=1, n_mels=1))


def test_6_refused_and_accepted_parameter_sets(fmrx):
    C, lib = fmrx.C, fmrx.lib
    x, st = np.zeros((2, 80), F32), np.zeros(1, fmrx.AUDIO_FEATURES_STATE_DTYPE)
    feat, frames = np.zeros((80, 128), F32), np.zeros(1, np.uint32)

    def params(**kw):
        return fmrx.AudioFeaturesParams(**dict(G0, **kw))

    def walk(p, ac=2, pitch=80, n=80, rows=x.ctypes.data, s=st.ctypes.data, f=feat.ctypes.data, fr=frames.ctypes.data, fill=0):
        st["fill"] = fill
        return lib.fmrx_audio_features_walk(None if p is None else C.byref(p), ac, rows, pitch, n, s, f, fr)

    h = C.c_void_p()
    w = np.zeros(1280, F32)
    for kw in GOOD:
        p = params(**kw)
        assert af.good({k: getattr(p, k) for k in af.FIELDS}) and walk(p) == fmrx.OK, kw
        assert fmrx.audioFeaturesMaxFrames(p, 80) == 79 // p.hop + 1
    for kw in BAD:
        p = params(**kw)
        assert not af.good({k: getattr(p, k) for k in af.FIELDS}), kw
        assert walk(p) == fmrx.EINVAL, kw
        assert lib.fmrx_audio_features_create(C.byref(h), C.byref(p), 1, 2, 1920, 0) == fmrx.EINVAL, kw      # refused before a device is asked for
        assert lib.fmrx_audio_features_max_frames(C.byref(p), 80) == 0, kw
        with pytest.raises(fmrx.FmrxError):
            fmrx.audioFeaturesTables(p)
    p = params()
    for bad in (dict(ac=0), dict(ac=3), dict(n=0), dict(pitch=79), dict(n=2 ** 26 + 1, pitch=2 ** 26 + 1), dict(rows=None), dict(s=None), dict(f=None),
                dict(fr=None), dict(fill=64), dict(fill=1279)):
        assert walk(p, **bad) == fmrx.EINVAL, bad
    assert walk(None) == fmrx.EINVAL and walk(p, fill=63) == fmrx.OK
    for bad in ((0, 2, 1920), (1, 0, 1920), (1, 3, 1920), (1, 2, 0), (1, 2, 2 ** 26 + 1)):
        assert lib.fmrx_audio_features_create(C.byref(h), C.byref(p), *bad, 0) == fmrx.EINVAL, bad
    assert lib.fmrx_audio_features_create(None, C.byref(p), 1, 2, 1920, 0) == fmrx.EINVAL
    assert lib.fmrx_audio_features_create(C.byref(h), None, 1, 2, 1920, 0) == fmrx.EINVAL
    assert lib.fmrx_audio_features_destroy(None) == fmrx.OK
    wp = w.ctypes.data
    for call in (lambda: lib.fmrx_audio_features_reset(None, 0), lambda: lib.fmrx_audio_features_state_get(None, None),
                 lambda: lib.fmrx_audio_features_process_dev(None, None, 0, 0, None), lambda: lib.fmrx_audio_features_collect(None, None, None),
                 lambda: lib.fmrx_audio_features_process(None, None, 0, 0, None, None), lambda: lib.fmrx_audio_features_result_dev(None, None, None),
                 lambda: lib.fmrx_audio_features_preset(48000.0, None), lambda: lib.fmrx_audio_features_tables(None, wp, wp, wp, wp, wp),
                 lambda: lib.fmrx_audio_features_tables(C.byref(p), None, wp, wp, wp, wp), lambda: lib.fmrx_audio_features_tables(C.byref(p), wp, wp, wp, wp, None)):
        assert call() == fmrx.EINVAL
    assert lib.fmrx_audio_features_max_frames(None, 80) == 0


def test_7_every_new_symbol_is_exported_and_mirrored(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_audio_features_\w+)\s*\(", text))
    assert declared == {"fmrx_audio_features_" + k for k in ("preset", "tables", "max_frames", "walk", "create", "destroy", "reset", "state_get",
                                                             "process_dev", "result_dev", "collect", "process")}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    for struct, size in (("params", 40), ("state", 5120)):
        assert f"sizeof(fmrx_audio_features_{struct}) == {size}" in text
    assert fmrx.C.sizeof(fmrx.AudioFeaturesParams) == 40 and fmrx.AUDIO_FEATURES_STATE_DTYPE.itemsize == 5120
    assert fmrx.AUDIO_FEATURES_STATE_DTYPE == af.STATE_DTYPE and tuple(n for n, _ in fmrx.AudioFeaturesParams._fields_) == af.FIELDS
    for name in ("AudioFeatures", "AudioFeaturesParams", "audioFeaturesPreset", "audioFeaturesTables", "audioFeaturesWalk", "audioFeaturesMaxFrames",
                 "AUDIO_FEATURES_STATE_DTYPE"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_bank", "process_dev", "process", "collect", "result_dev", "state", "reset", "close"):
        assert hasattr(fmrx.AudioFeatures, name), name
