"""The audio rate converter without a GPU (include/fmrx.h: fmrx_audio_resample_*): the taps against a numpy
float64 restatement and their frequency response, the host walk against the model bit for bit, that the samples do not depend on how
a stream is cut into calls, the model against a float64 zero-stuff / convolve / decimate reference, tones through the 48 -> 16 kHz
preset, the refusals and the exported symbols."""
import ctypes as C
import re

import numpy as np
import pytest

import _audio_resample_model as ar

F32, F64 = np.float32, np.float64
GEOMETRIES = {"1/3": ar.preset(48000, 16000), "147/160": ar.preset(48000, 44100), "160/441": ar.preset(44100, 16000), "3/7": ar.G_SMALL}
_taps = {}


def params(fmrx, g):
    return fmrx.AudioResampleParams(**g)


def taps(fmrx, g):
    key = tuple(g[k] for k in ar.FIELDS if k != "mix")
    if key not in _taps:
        _taps[key] = fmrx.audioResampleTaps(g)
    return _taps[key]


def host_walk(fmrx, x, g, state=None, pitch=None):
    """fmrx_audio_resample_walk channel by channel on rows [N][ac][n], at a pitch of its own -> as the model's walk"""
    N, ac, n = x.shape
    pitch = n if pitch is None else pitch
    state = ar.fresh(N) if state is None else state.copy()
    R, m_max = ar.rows_of(g, ac), ar.max_out(n, g)
    out, counts = np.zeros((N, R, m_max), F32), np.zeros(N, np.uint32)
    p = params(fmrx, g)
    for c in range(N):
        rows = np.full((ac, pitch), 3e38, F32)
        rows[:, :n] = x[c]
        o, cnt = np.full((R, m_max), 7.0, F32), np.zeros(1, np.uint32)
        st = state[c:c + 1].copy()
        rc = fmrx.lib.fmrx_audio_resample_walk(C.byref(p), ac, rows.ctypes.data, pitch, n, st.ctypes.data, o.ctypes.data, cnt.ctypes.data)
        assert rc == fmrx.OK
        out[c], counts[c], state[c] = o, cnt[0], st[0]
    return out, counts, state


# ---- taps -----------------------------------------------------------------------------------------------------------------
def test_1_the_preset_gives_the_table_of_the_issue(fmrx):
    for (fi, fo), (up, down, T) in ar.PRESETS.items():
        for mix in (0, 1):
            p = fmrx.AudioResampleParams.preset(fi, fo, mix)
            got = {k: getattr(p, k) for k in ar.FIELDS}
            assert got == ar.preset(fi, fo, mix) == ar.geometry(up, down, T, mix), (fi, fo)
            assert fmrx.audioResampleLatency(p) == ar.latency(got) == (up * T - 1) / (2.0 * up)
            assert fmrx.audioResampleMaxOut(p, 1920) == -(-1920 * up // down)
    assert fmrx.audioResampleMaxOut(fmrx.AudioResampleParams(160, 1, 8, 1, 0.9, 8.0), 2 ** 26) == 160 * 2 ** 26       # beyond 2^32: 64-bit


@pytest.mark.parametrize("name", [f"{a}->{b}" for a, b in ar.PRESETS] + ["3/7"])
def test_1_taps_equal_the_formula_to_one_ulp(fmrx, name):
    """the library sums I0's power series and calls libm's sin; formula() uses numpy's Chebyshev I0 and its sinc: both are good to a few
    ulp of float64, so the float32 roundings differ only where the float64 value sits at a rounding boundary: at most 1 ulp of float32"""
    g = ar.G_SMALL if name == "3/7" else ar.preset(*map(int, name.split("->")))
    h, f = taps(fmrx, g), ar.formula(g)
    assert h.shape == f.shape == (g["up"], g["taps"]) and h.dtype == F32
    ulp = np.spacing(np.maximum(np.abs(h), np.abs(f)))
    assert (np.abs(h.astype(F64) - f.astype(F64)) <= ulp).all()
    assert (h.view(np.uint32) == f.view(np.uint32)).mean() > 0.95
    dc = h.astype(F64).sum(axis=1)
    print(name, "dc gain of the phases", dc.min(), dc.max())
    if name != "3/7":                  # every preset; eight taps at 3/7 are 1.7 zero crossings a side, and the formula itself sums to 0.924 there
        assert (np.abs(dc - 1.0) <= 1e-4).all()
    proto = np.ascontiguousarray(h.T).reshape(-1)                                                                   # g[j up + p]
    assert np.array_equal(proto, proto[::-1])                                                                       # linear phase


@pytest.mark.parametrize("rates", list(ar.PRESETS))
def test_1_frequency_response_of_every_presets_prototype(fmrx, rates):
    """the FFT of g at the rate in * up, divided by up; ny = min(in, out) / 2.  On the library's float32 taps"""
    fi, fo = rates
    g = ar.preset(fi, fo)
    U = g["up"]
    proto = np.ascontiguousarray(taps(fmrx, g).astype(F64).T).reshape(-1)
    nfft = 1 << 21
    H = np.abs(np.fft.rfft(proto, nfft)) / U
    f = np.arange(len(H)) * (fi * U / nfft)
    ny = min(fi, fo) / 2.0
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    pas, s60, s80 = db[f <= 0.75 * ny], db[f >= 1.1 * ny], db[f >= 1.25 * ny]
    print(rates, "passband", pas.max(), pas.min(), "from 1.1 ny", s60.max(), "from 1.25 ny", s80.max())
    assert pas.max() <= 0.005 and pas.min() >= -0.2
    assert s60.max() <= -60.0
    assert s80.max() <= -80.0


# ---- walk against model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("mix", [0, 1])
@pytest.mark.parametrize("ac", [1, 2])
def test_2_the_host_walk_equals_the_model(fmrx, ac, mix, name):
    g = dict(GEOMETRIES[name], mix=mix)
    T = g["taps"]
    h = taps(fmrx, g)
    rng = np.random.default_rng(200 + 10 * ac + mix + len(name))
    N = 3
    sm, sh = ar.fresh(N), ar.fresh(N)
    total = 0
    for call, n in enumerate((1920, 1, T - 2, T - 1, 1920, 1)):
        x = (0.9 * rng.standard_normal((N, ac, n))).astype(F32)
        want, counts, sm = ar.walk(x, sm, g, h)
        got, got_counts, sh = host_walk(fmrx, x, g, sh, pitch=n + 5)       # pitched rows, 3e38 behind every row
        assert np.array_equal(got_counts, counts) and ar.same(got, want) and ar.same(sh, sm), (call, n)
        assert np.isfinite(got).all() and not got[:, :, counts[0]:].view(np.uint32).any()
        total += int(counts[0])
        fed = sum((1920, 1, T - 2, T - 1, 1920, 1)[:call + 1])
        assert total == ar.outputs_of(fed, g, 0) and sm["pos"][0] == total * g["down"] - fed * g["up"]      # the calls continue one stream
        assert not sm["carry"][:, ar.rows_of(g, ac):].any() and not sm["carry"][:, :, T - 1:].any()


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac", [1, 2])
def test_2_special_values_at_window_and_call_boundaries(fmrx, ac, name):
    """+-0, denormals, +-infinity, NaN and +-FLT_MAX at the calls' first and last samples and T - 1 and T from either end, over three
    calls, so that every one of them is also read out of the carried state"""
    T = GEOMETRIES[name]["taps"]
    rng = np.random.default_rng(260 + ac + len(name))
    N = 7
    for mix in (0, 1):
        g = dict(GEOMETRIES[name], mix=mix)
        h = taps(fmrx, g)
        sm, sh = ar.fresh(N), ar.fresh(N)
        seen = np.zeros(3, bool)
        for call, n in enumerate((2 * T + 3, T - 1, 3 * T)):
            x = ar.special_rows(rng, N, ac, n, T)
            want, counts, sm = ar.walk(x, sm, g, h)
            got, got_counts, sh = host_walk(fmrx, x, g, sh)
            assert np.array_equal(got_counts, counts) and ar.same(got, want) and ar.same(sh, sm), (mix, call)
            seen |= [np.isnan(want).any(), np.isinf(want).any(), (np.isfinite(want).all(axis=(1, 2))).any()]
        assert seen.all()


def test_2_a_nan_reaches_exactly_the_outputs_whose_window_holds_it(fmrx):
    for name, g in GEOMETRIES.items():
        U, D, T = g["up"], g["down"], g["taps"]
        n, s = 6 * T, 2 * T + 1
        x = np.ones((1, 1, n), F32)
        x[0, 0, s] = np.nan
        y, counts, _ = host_walk(fmrx, x, g)
        i = (np.arange(counts[0]) * D) // U
        holds = (i >= s) & (i - s < T)
        assert np.array_equal(np.isnan(y[0, 0, :counts[0]]), holds), name
        assert holds.sum() >= (T * U) // D - 1                         # (a zero tap would still give NaN: 0 * NaN)


# ---- split invariance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("ac,mix", [(1, 1), (2, 1), (2, 0)])
def test_3_one_call_equals_the_same_stream_in_other_calls(fmrx, ac, mix, name):
    g = dict(GEOMETRIES[name], mix=mix)
    T, n = g["taps"], 5000
    rng = np.random.default_rng(300 + ac + mix + len(name))
    x = (0.9 * rng.standard_normal((2, ac, n))).astype(F32)
    whole, counts, st = host_walk(fmrx, x, g)
    parts, state, a, total = [], ar.fresh(2), 0, 0
    for k in (1, 7, T - 2, 1920, n):
        k = min(k, n - a)
        out, cnt, state = host_walk(fmrx, x[:, :, a:a + k], g, state)
        assert cnt[0] == cnt[1]
        parts.append(out[:, :, :cnt[0]])
        a, total = a + k, total + int(cnt[0])
    assert a == n and total == counts[0] == ar.max_out(n, g)
    assert np.concatenate(parts, axis=2).tobytes() == whole[:, :, :counts[0]].tobytes()
    assert state.tobytes() == st.tobytes()
    if name == "1/3":                                                  # and the model cuts the same way
        want, wc, ws = ar.walk(x, ar.fresh(2), g, taps(fmrx, g))
        assert ar.same(whole, want) and ar.same(st, ws)


# ---- against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_4_the_model_against_a_float64_reference(fmrx, name):
    """|y - y64| <= (T + 2) 2^-24 sum_j |h[p][j]| |x[i - j]| per output: an fma chain of T steps errs by at most T u times the sum of the
    magnitudes to first order (u = 2^-24), the mix's one rounding adds u of it, and one more u covers the second-order terms"""
    g = GEOMETRIES[name]
    T = g["taps"]
    h = taps(fmrx, g)
    n = 400 if g["up"] > 3 else 3000
    rng = np.random.default_rng(400 + len(name))
    x = (0.9 * rng.standard_normal((1, 2, n))).astype(F32)
    y, counts, _ = host_walk(fmrx, x, g)
    xm = 0.5 * (x[0, 0].astype(F64) + x[0, 1].astype(F64))             # the mix in float64
    y64, mag = ar.reference64(xm, h, g)
    assert counts[0] == len(y64)
    err = np.abs(y[0, 0, :counts[0]].astype(F64) - y64)
    bound = (T + 2) * 2.0 ** -24 * mag
    print(name, "worst error / bound", (err / bound).max())
    assert (err <= bound).all()
    assert err.max() > 0                                               # float32 shows


# ---- tones ----------------------------------------------------------------------------------------------------------------
def test_5_tones_through_the_48_to_16_khz_preset(fmrx):
    g = ar.preset(48000, 16000)
    T, n, lat = g["taps"], 9600, ar.latency(g)
    s = np.arange(n, dtype=F64)
    x = np.sin(2 * np.pi * 1000.0 * s / 48000.0).astype(F32).reshape(1, 1, n)
    y, counts, _ = host_walk(fmrx, x, g)
    m = np.arange(2 * T, counts[0])
    want = np.sin(2 * np.pi * 1000.0 * (3.0 * m - lat) / 48000.0)      # the same sine at 16 kHz, delayed by the latency (input samples)
    err = np.abs(y[0, 0, m] - want).max()
    print("1 kHz: worst error", err)
    assert err <= 2e-3
    x = np.sin(2 * np.pi * 10500.0 * s / 48000.0).astype(F32).reshape(1, 1, n)
    y, counts, _ = host_walk(fmrx, x, g)
    rms = np.sqrt(np.mean(y[0, 0, 2 * T:counts[0]].astype(F64) ** 2))
    print("10.5 kHz: rms", rms)
    assert rms <= 1e-4


# ---- refusals and ABI -----------------------------------------------------------------------------------------------------
GOOD = (dict(), dict(up=160, down=1, taps=100), dict(up=1, down=1024, taps=256), dict(up=64, down=1023, taps=256), dict(taps=8), dict(mix=0),
        dict(cutoff=1.0), dict(cutoff=1e-3), dict(beta=0.0), dict(beta=20.0))
BAD = (dict(up=0), dict(up=161, down=160), dict(down=0), dict(down=1025), dict(up=2, down=4), dict(up=3, down=3), dict(taps=4), dict(taps=260),
       dict(taps=10), dict(up=160, down=1, taps=104), dict(mix=2), dict(cutoff=0.0), dict(cutoff=-0.5), dict(cutoff=1.0001), dict(cutoff=float("nan")),
       dict(cutoff=float("inf")), dict(beta=-0.1), dict(beta=20.5), dict(beta=float("nan")), dict(beta=float("inf")))


def test_6_every_limit_is_refused(fmrx):
    lib = fmrx.lib
    x = np.zeros((2, 80), F32)
    st = np.zeros(1, ar.STATE_DTYPE)
    out, cnt = np.zeros((2, 80 * 160), F32), np.zeros(1, np.uint32)

    def params(**kw):
        return fmrx.AudioResampleParams(**dict(ar.G_SMALL, **kw))

    def walk(p, ac=2, pitch=80, n=80, rows=x.ctypes.data, s=st.ctypes.data, o=out.ctypes.data, c=cnt.ctypes.data, pos=0):
        st["pos"] = pos
        return lib.fmrx_audio_resample_walk(None if p is None else C.byref(p), ac, rows, pitch, n, s, o, c)

    h = C.c_void_p()
    w = np.zeros(16384, F32)
    for kw in GOOD:
        p = params(**kw)
        assert walk(p) == fmrx.OK, kw
        assert fmrx.audioResampleMaxOut(p, 80) == -(-80 * p.up // p.down) and fmrx.audioResampleTaps(p).shape == (p.up, p.taps)
    for kw in BAD:
        p = params(**kw)
        assert walk(p) == fmrx.EINVAL, kw
        assert lib.fmrx_audio_resample_create(C.byref(h), C.byref(p), 1, 2, 1920, 1, 0, 0) == fmrx.EINVAL, kw      # refused before a device is asked for
        assert lib.fmrx_audio_resample_max_out(C.byref(p), 80) == 0, kw
        assert np.isnan(lib.fmrx_audio_resample_latency(C.byref(p))), kw
        assert lib.fmrx_audio_resample_taps(C.byref(p), w.ctypes.data) == fmrx.EINVAL, kw
    p = params()
    for bad in (dict(ac=0), dict(ac=3), dict(n=0), dict(pitch=79), dict(n=2 ** 26 + 1, pitch=2 ** 26 + 1), dict(rows=None), dict(s=None), dict(o=None),
                dict(c=None), dict(pos=7), dict(pos=2 ** 31)):
        assert walk(p, **bad) == fmrx.EINVAL, bad
    assert walk(None) == fmrx.EINVAL and walk(p, pos=6) == fmrx.OK
    assert lib.fmrx_audio_resample_create(C.byref(h), C.byref(p), 1, 2, 1920, 0, 0, 0) == fmrx.EINVAL              # neither result
    assert lib.fmrx_audio_resample_create(None, C.byref(p), 1, 2, 1920, 1, 0, 0) == fmrx.EINVAL
    assert lib.fmrx_audio_resample_create(C.byref(h), None, 1, 2, 1920, 1, 0, 0) == fmrx.EINVAL
    for bad in ((0, 2, 1920), (1, 0, 1920), (1, 3, 1920), (1, 2, 0), (1, 2, 2 ** 26 + 1)):
        assert lib.fmrx_audio_resample_create(C.byref(h), C.byref(p), *bad, 1, 1, 0) == fmrx.EINVAL, bad
    assert lib.fmrx_audio_resample_destroy(None) == fmrx.OK
    wp = w.ctypes.data
    for call in (lambda: lib.fmrx_audio_resample_reset(None, 0), lambda: lib.fmrx_audio_resample_state_get(None, None),
                 lambda: lib.fmrx_audio_resample_process_dev(None, None, 0, 0, 1, None), lambda: lib.fmrx_audio_resample_collect(None, None, None, None),
                 lambda: lib.fmrx_audio_resample_process(None, None, 0, 0, 1, None, None, None),
                 lambda: lib.fmrx_audio_resample_result_dev(None, None, None, None), lambda: lib.fmrx_audio_resample_preset(48000.0, 16000.0, 1, None),
                 lambda: lib.fmrx_audio_resample_taps(None, wp), lambda: lib.fmrx_audio_resample_taps(C.byref(p), None)):
        assert call() == fmrx.EINVAL
    assert lib.fmrx_audio_resample_max_out(None, 80) == 0 and lib.fmrx_audio_resample_max_out(C.byref(p), 0) == 0
    assert np.isnan(lib.fmrx_audio_resample_latency(None))


def test_6_the_preset_refuses_other_rates(fmrx):
    q = fmrx.AudioResampleParams()
    for fi, fo, mix in ((7999, 16000, 1), (48000, 48001, 1), (48000.5, 16000, 1), (48000, 16000.25, 1), (float("nan"), 16000, 1), (48000, float("inf"), 1),
                        (48000, 47999, 1), (44100, 32000, 1), (48000, 16000, 2), (48000, 16000, -1)):
        assert fmrx.lib.fmrx_audio_resample_preset(float(fi), float(fo), mix, C.byref(q)) == fmrx.EINVAL, (fi, fo, mix)      # 320/441 is beyond up's limit
    for fi, fo in ((48000, 48000), (8000, 48000), (44100, 8000), (32000, 16000), (48000, 12000)):
        p = fmrx.AudioResampleParams.preset(fi, fo)
        assert {k: getattr(p, k) for k in ar.FIELDS} == ar.preset(fi, fo), (fi, fo)


def test_7_every_new_symbol_is_exported_and_mirrored(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_audio_resample_\w+)\s*\(", text))
    assert declared == {"fmrx_audio_resample_" + k for k in ("preset", "taps", "max_out", "latency", "walk", "create", "destroy", "reset", "state_get",
                                                             "process_dev", "result_dev", "collect", "process")}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(fmrx_audio_resample_\w+)", nm)) == declared
    for struct, size in (("params", 32), ("state", 2048)):
        assert f"sizeof(fmrx_audio_resample_{struct}) == {size}" in text
    assert fmrx.C.sizeof(fmrx.AudioResampleParams) == 32 and fmrx.AUDIO_RESAMPLE_STATE_DTYPE.itemsize == 2048
    assert fmrx.AUDIO_RESAMPLE_STATE_DTYPE == ar.STATE_DTYPE and tuple(n for n, _ in fmrx.AudioResampleParams._fields_) == ar.FIELDS
