"""The audio spectrum meter without a GPU (include/fmrx.h: fmrx_audio_spectrum_*): the tables against
their committed bits and the formula, the host walk against the model bit for bit, how the cut of a stream into calls shows in
the sums, the model against a float64 FFT, full-scale sines, the edge rules of the levels, the refusals and the exported symbols."""
import re

import numpy as np
import pytest

import _audio_spectrum_model as sp

F32, F64 = np.float32, np.float64


def bits(a):
    return [f"{v:08x}" for v in np.asarray(a, F32).view(np.uint32)]


# ---- the tables ---------------------------------------------------------------------------------------------------------
def test_1_the_tables_equal_their_bits_the_formula_and_the_library(fmrx):
    assert sp.W.shape == sp.C.shape == (256,) and sp.W.dtype == sp.C.dtype == F32
    assert bits(sp.C[:65]) == sp.C_BITS.split() and bits(sp.W[:129]) == sp.W_BITS.split()
    assert [bits(sp.C)[m] for m in (0, 1, 2, 32, 63)] == ["3f800000", "3f7fec43", "3f7fb10f", "3f3504f3", "3cc90ab0"]
    w, c = sp.formula()
    assert bits(w) == bits(sp.W) and bits(c) == bits(sp.C)
    wd, cd = sp.direct()                      # no symmetry: the same everywhere but at the cosine's two zeros
    assert bits(wd) == bits(sp.W)
    assert [m for m in range(256) if bits(cd)[m] != bits(sp.C)[m]] == [64, 192]
    assert bits(sp.C[[64, 192]]) == ["00000000"] * 2 and bits(sp.W[:1]) == ["00000000"] and sp.C[128] == -1.0 and sp.W[128] == 1.0
    lw, lc = fmrx.audioSpectrumTables()
    assert bits(lw) == bits(sp.W) and bits(lc) == bits(sp.C)
    lib = fmrx.lib
    assert (lib.fmrx_audio_spectrum_frame(), lib.fmrx_audio_spectrum_bins(), lib.fmrx_audio_spectrum_tile(), lib.fmrx_audio_spectrum_max_bands()) == \
        (sp.FRAME, sp.BINS, sp.TILE, sp.MAX_BANDS) == (256, 128, 16, 32)
    assert tuple(fmrx.audioSpectrumDefaultEdges()) == sp.DEFAULT_EDGES and len(sp.DEFAULT_EDGES) == 24
    assert sp.DEFAULT_EDGES[21] <= 19000.0 / 187.5 < sp.DEFAULT_EDGES[22]                      # the pilot falls in band 21
    assert abs(256.0 * float((sp.W.astype(F64) ** 2).sum()) / 4.0 - sp.NORM) < 1e-4            # 6144 = 256 sum(w^2) / 4


# ---- the host walk ------------------------------------------------------------------------------------------------------
def host_walk(fmrx, rows, states, edges=None):
    """fmrx_audio_spectrum_walk channel by channel, in the model's shapes; states is replaced"""
    rec = np.zeros(rows.shape[0], fmrx.AUDIO_SPECTRUM_DTYPE)
    for c in range(rows.shape[0]):
        rec[c], states[c] = fmrx.audioSpectrumWalk(rows[c], states[c], edges)
    return rec


EDGES = {"default": None, "one band": (1, 128), "32 bands": tuple(range(1, 32)) + (40, 128)}
CALLS = (1, 255, 256, 257, 1920, 4097)


@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("ac", [1, 2])
def test_2_the_host_walk_equals_the_model_bit_for_bit(fmrx, ac, edges):
    N, e = 4, EDGES[edges]
    assert fmrx.AUDIO_SPECTRUM_DTYPE == sp.AUDIO_SPECTRUM_DTYPE and fmrx.AUDIO_SPECTRUM_STATE_DTYPE == sp.AUDIO_SPECTRUM_STATE_DTYPE
    B = len(sp.check_edges(e)) - 1
    assert B == {"default": 23, "one band": 1, "32 bands": 32}[edges]
    rng = np.random.default_rng(10 * ac + B)
    model, states = sp.fresh(N), sp.fresh(N)
    fill, seen_nan = 0, False
    for call, n in enumerate(CALLS):
        x = sp.special_rows(rng, N, ac, n)
        if n >= 256:
            x[-2, 0, n // 2] = np.nan                                                  # a NaN: its frame reads NaN
            x[-1, ac - 1, 100], x[-1, ac - 1, 103] = np.inf, -np.inf                   # both infinities inside one frame
        x[0, 0, :] = rng.choice(np.array([1e-40, -3e-45, 1.17549435e-38, -0.0, 0.0], F32), n)      # a row of denormals and zeros alone
        want, model = sp.walk(x, model, e)
        got = host_walk(fmrx, x, states, e)
        assert sp.same(got, want), (call, n)
        assert sp.same(states, model), (call, n)
        F, fill = divmod(fill + n, 256)
        assert (got["n"] == n).all() and (got["frames"] == F).all() and (states["fill"] == fill).all()
        assert not got["band"][:, ac:].any() and not got["band"][:, :, B:].any()
        assert not states["carry"][:, :, fill:].any() and not states["carry"][:, ac:].any()
        if F == 0:
            assert not got["band"].any()
        else:
            assert np.isfinite(got["band"][:2]).all() and (got["band"][1, :ac, :B] > 0).all()
        if n >= 256:
            seen_nan |= bool(np.isnan(want["band"][-2, 0, :B]).all() and not np.isfinite(want["band"][-1, ac - 1, :B]).any())
    assert seen_nan


def test_2_denormal_windowed_samples_and_products_are_kept(fmrx):
    x = np.zeros((1, 256), F32)
    x[0, 100], x[0, 7] = F32(1e-20), F32(1e-40)        # 1e-20 squares into the denormal range; 1e-40 w[7] is itself denormal
    rec, _ = fmrx.audioSpectrumWalk(x, None, (1, 128))
    want, _ = sp.walk(x[None], sp.fresh(1), (1, 128))
    assert sp.same(rec, want[0])
    p = sp.bin_powers(x[0])
    assert ((p > 0) & (p < np.finfo(F32).tiny)).sum() >= 100 and 0 < rec["band"][0, 0] < 128 * float(np.finfo(F32).tiny)
    y = np.zeros((1, 256), F32)
    y[0, 7] = F32(1e-40)
    xw = y[0] * sp.W
    assert 0 < xw[7] < np.finfo(F32).tiny
    rec, _ = fmrx.audioSpectrumWalk(y, None, (1, 128))
    assert sp.same(rec, sp.walk(y[None], sp.fresh(1), (1, 128))[0][0]) and rec["band"][0, 0] == 0.0      # the squares underflow; the chains did not flush


def test_2_a_non_finite_sample_leaves_no_finite_bin_in_its_frame(fmrx):
    """a NaN makes every bin NaN; an infinity makes every bin NaN or infinite: NaN wherever it meets one of the tables' zeros
    (w[0], C[64], C[192]), infinity elsewhere"""
    for v in (np.nan, np.inf, -np.inf):
        for j in (0, 1, 64, 255):
            x = np.ones((1, 512), F32)
            x[0, 256 + j] = v
            p = sp.bin_powers(x[0].reshape(2, 256))
            assert np.isfinite(p[0]).all() and not np.isfinite(p[1]).any(), (v, j)
            if np.isnan(v) or j in (0, 64):
                assert np.isnan(p[1]).all(), (v, j)
            rec, _ = fmrx.audioSpectrumWalk(x)
            assert sp.same(rec, sp.walk(x[None], sp.fresh(1))[0][0]) and not np.isfinite(rec["band"][0, :23]).any() and rec["frames"] == 2


# ---- cutting the stream -------------------------------------------------------------------------------------------------
def test_3_calls_of_one_frame_give_the_frames_powers_and_one_call_the_two_level_sum(fmrx):
    rng = np.random.default_rng(3)
    F = 37                                                           # two full tiles and one of five frames
    x = (0.5 * rng.standard_normal((2, F * 256 + 100))).astype(F32)
    bp = sp.band_powers(sp.bin_powers(x[:, :F * 256].reshape(2, F, 256)))          # [2][F][23] float32
    st = None
    for f in range(F):
        rec, st = fmrx.audioSpectrumWalk(x[:, 256 * f:256 * f + 256], st)
        assert rec["frames"] == 1 and st["fill"] == 0
        assert sp.same(rec["band"][:, :23], bp[:, f].astype(F64)), f
    whole, st = fmrx.audioSpectrumWalk(x)
    assert whole["frames"] == F and st["fill"] == 100 and np.array_equal(st["carry"][:, :100], x[:, F * 256:])
    two = sp.two_level(np.moveaxis(bp, 1, 0))
    assert sp.same(whole["band"][:, :23], two)
    flat = np.zeros((2, 23))
    for f in range(F):
        flat = flat + bp[:, f].astype(F64)
    assert np.allclose(two, flat, rtol=1e-14, atol=0)      # the grouping can show in the last bits only (float32 terms in float64: often not at all)
    # a cut that is no multiple of the frame: the frames' powers are the same, another grouping
    st, parts = None, np.zeros((2, 23))
    for a, b in ((0, 1000), (1000, 1001), (1001, 5000), (5000, x.shape[1])):
        rec, st = fmrx.audioSpectrumWalk(x[:, a:b], st)
        parts = parts + rec["band"][:, :23]
    assert st["fill"] == 100 and np.allclose(parts, two, rtol=1e-14, atol=0)


# ---- against a float64 FFT ----------------------------------------------------------------------------------------------
def fft_powers(frames) -> np.ndarray:
    """|rfft|^2 of the float64 windowed frames, bins 0 .. 127"""
    xw = np.asarray(frames, F32).astype(F64) * sp.W.astype(F64)
    return (np.abs(np.fft.rfft(xw, axis=-1)) ** 2)[..., :128]


def fft_bands(p64, edges=None) -> np.ndarray:
    e = sp.check_edges(edges)
    return np.stack([p64[..., e[b]:e[b + 1]].sum(axis=-1) for b in range(len(e) - 1)], axis=-1)


@pytest.mark.parametrize("kind", ["noise", "noise and a tone"])
def test_4_bins_and_bands_against_a_float64_fft(kind):
    worst_bin, worst_band = 0.0, 0.0
    for seed in range(6):
        rng = np.random.default_rng(40 + seed)
        x = 0.5 * rng.standard_normal((8, 256))
        if kind != "noise":
            x += 1.5 * np.sin(2.0 * np.pi * (20.3 + 11.0 * seed) * np.arange(256) / 256.0 + seed)
        x = x.astype(F32)
        p, p64 = sp.bin_powers(x), fft_powers(x)
        worst_bin = max(worst_bin, float((np.abs(p - p64).max(axis=1) / p64.max(axis=1)).max()))
        b, b64 = sp.band_powers(p), fft_bands(p64)
        worst_band = max(worst_band, float((np.abs(b - b64).max(axis=1) / b64.max(axis=1)).max()))
    print(f"{kind}: worst bin error {worst_bin:.2e} of the frame's largest bin, worst band error {worst_band:.2e} of its largest band")
    assert worst_bin <= 1e-5 and worst_band <= 1e-5


# ---- sines --------------------------------------------------------------------------------------------------------------
def sine(bins, frames=16, amplitude=sp.FULL_SCALE):
    j = np.arange(256 * frames, dtype=F64)
    return (amplitude * np.sin(2.0 * np.pi * bins * j / 256.0 + 0.3)).astype(F32)[None]


TONES = {44.0: 16, 44.25: 16, 44.5: 16, 101.33: 21, 120.0: 22}       # bins -> the default band that holds the tone (at least 8 wide)


@pytest.mark.parametrize("bins", list(TONES))
def test_5_a_full_scale_sine_reads_0_dbfs_in_total_and_in_its_band(fmrx, bins):
    b = TONES[bins]
    e = sp.DEFAULT_EDGES
    assert e[b] + 2 <= bins <= e[b + 1] - 3 and e[b + 1] - e[b] >= 8
    rec, _ = fmrx.audioSpectrumWalk(sine(bins))
    lv = fmrx.audioSpectrumDerive(rec, 1)
    print(f"{bins} bins: total {lv['total_dbfs'][0]:+.2e} dB, band {b} {lv['band_dbfs'][0, b]:+.2e} dB")
    assert abs(lv["total_dbfs"][0]) <= 0.001 and abs(lv["band_dbfs"][0, b]) <= 0.001
    assert lv["total_dbfs"][1] == -99.0 and (lv["band_dbfs"][1] == -99.0).all() and (lv["band_dbfs"][0, 23:] == -99.0).all()
    fc = (e[b] + e[b + 1] - 1) / 2.0 * 187.5
    assert abs(lv["centroid_hz"][0] - fc) <= 0.001 * fc and lv["centroid_hz"][1] == 0.0     # a single tone: its band's centre


def test_5_a_sine_at_one_bin_reads_what_the_float64_fft_gives(fmrx):
    x = sine(1.0)
    rec, _ = fmrx.audioSpectrumWalk(x)
    got = fmrx.audioSpectrumDerive(rec, 1)["total_dbfs"][0]
    p64 = fft_powers(x[0].reshape(16, 256))
    want = 10.0 * np.log10(p64[:, 1:].sum(axis=1).mean() / (sp.NORM * 4.0))
    print(f"1.0 bin: total {got:.4f} dB, the float64 FFT {want:.4f} dB")
    assert abs(got - want) <= 0.001 and -0.9 < want < -0.7            # bin 0 holds part of it


# ---- the levels ---------------------------------------------------------------------------------------------------------
def record(**kw):
    r = np.zeros((), sp.AUDIO_SPECTRUM_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def levels(fmrx, rec, ac, edges=None, Fs=48000.0, fs=2.0):
    got, want = fmrx.audioSpectrumDerive(rec, ac, edges, Fs, fs), sp.derive(rec, ac, edges, Fs, fs)
    assert set(got) == set(want)
    for k in got:
        assert got[k].shape == want[k].shape and np.allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True), (k, got[k], want[k])
    return got


def test_6_the_levels_and_their_edge_rules(fmrx):
    band = np.zeros((2, 32))
    band[0, 16], band[1, 3], band[1, 22] = 10 * 6144.0 * 4.0, 10 * 6144.0, 10 * 6144.0
    lv = levels(fmrx, record(n=2560, frames=10, band=band), 2)
    assert lv["band_dbfs"][0, 16] == 0.0 and lv["total_dbfs"][0] == 0.0 and abs(lv["band_dbfs"][1, 3] - -6.0206) < 1e-4
    assert abs(lv["total_dbfs"][1] - -3.0103) < 1e-4 and lv["band_dbfs"][0, 0] == -99.0
    assert lv["centroid_hz"][0] == 43.5 * 187.5 and lv["centroid_hz"][1] == (4.0 + 119.5) / 2.0 * 187.5
    mono = levels(fmrx, record(n=2560, frames=10, band=band), 1)                    # the second row is not read
    assert (mono["band_dbfs"][1] == -99.0).all() and mono["total_dbfs"][1] == -99.0 and mono["centroid_hz"][1] == 0.0
    zero = levels(fmrx, record(n=7, frames=0, band=band), 2)                        # no frame completed
    assert (zero["band_dbfs"] == -99.0).all() and (zero["total_dbfs"] == -99.0).all() and not zero["centroid_hz"].any()
    dead = levels(fmrx, record(n=2560, frames=10), 2)                               # zero total: the floor, centroid 0
    assert (dead["band_dbfs"] == -99.0).all() and (dead["total_dbfs"] == -99.0).all() and not dead["centroid_hz"].any()
    nan = band.copy()
    nan[0, 16] = np.nan
    lv = levels(fmrx, record(n=2560, frames=10, band=nan), 2)                       # a NaN band: the floor there and in the total
    assert lv["band_dbfs"][0, 16] == -99.0 and lv["total_dbfs"][0] == -99.0 and lv["centroid_hz"][0] == 0.0 and lv["centroid_hz"][1] > 0
    huge = np.zeros((2, 32))
    huge[0, 0], huge[1, 0] = np.inf, 1e-300
    lv = levels(fmrx, record(n=256, frames=1, band=huge), 2)
    assert lv["band_dbfs"][0, 0] == 99.0 and lv["band_dbfs"][1, 0] == -99.0
    one = levels(fmrx, record(n=2560, frames=10, band=band), 2, edges=(1, 128), Fs=32000.0, fs=1.0)      # bands >= B are not read
    assert (one["band_dbfs"][:, 1:] == -99.0).all() and one["centroid_hz"][1] == 0.0 and one["centroid_hz"][0] == 0.0
    for bad in (dict(fs=0.0), dict(fs=float("nan")), dict(Fs=0.0), dict(Fs=float("inf")), dict(ac=3), dict(edges=(2, 2)), dict(edges=(0, 5))):
        kw = dict(ac=2, edges=None, Fs=48000.0, fs=2.0)
        kw.update(bad)
        with pytest.raises(fmrx.FmrxError):
            fmrx.audioSpectrumDerive(record(), kw["ac"], kw["edges"], kw["Fs"], kw["fs"])


# ---- the interface ------------------------------------------------------------------------------------------------------
BAD_EDGES = ((1, 1), (5, 4), (1, 2, 2, 3), (0, 4), (1, 129), (-1, 3), (1,), tuple(range(1, 35)))      # the last two: B = 0, B = 33


def test_7_refused_and_accepted_parameter_sets(fmrx):
    x, st, rec = np.zeros((2, 16), F32), np.zeros(1, fmrx.AUDIO_SPECTRUM_STATE_DTYPE), np.zeros(1, fmrx.AUDIO_SPECTRUM_DTYPE)

    def walk(ac, pitch, n, edges=None, rows=x.ctypes.data, s=st.ctypes.data, r=rec.ctypes.data):
        e = None if edges is None else np.array(edges, np.int32)
        st["fill"] = 0
        return fmrx.lib.fmrx_audio_spectrum_walk(ac, rows, pitch, n, None if e is None else e.ctypes.data, 0 if e is None else len(e) - 1, s, r)

    for ok in ((1, 16, 16), (2, 16, 16), (2, 16, 1), (2, 16, 16, (1, 128)), (2, 16, 16, (127, 128)), (1, 16, 16, tuple(range(1, 34)))):
        assert walk(*ok) == fmrx.OK, ok
    for bad in ((0, 16, 16), (3, 16, 16), (2, 16, 0), (2, 15, 16), (1, 2 ** 26 + 1, 2 ** 26 + 1)) + tuple((2, 16, 16, e) for e in BAD_EDGES):
        assert walk(*bad) == fmrx.EINVAL, bad
    assert walk(1, 16, 16, rows=None) == fmrx.EINVAL and walk(1, 16, 16, s=None) == fmrx.EINVAL and walk(1, 16, 16, r=None) == fmrx.EINVAL
    st["fill"] = 256
    assert fmrx.lib.fmrx_audio_spectrum_walk(1, x.ctypes.data, 16, 16, None, 0, st.ctypes.data, rec.ctypes.data) == fmrx.EINVAL
    h = fmrx.C.c_void_p()

    def create(N, ac, n_audio, edges=None):
        e = None if edges is None else np.array(edges, np.int32)
        return fmrx.lib.fmrx_audio_spectrum_create(fmrx.C.byref(h), N, ac, n_audio, None if e is None else e.ctypes.data, 0 if e is None else len(e) - 1, 0)

    # parameter sets the create call refuses before it asks for a device
    for bad in ((0, 2, 1920), (1, 0, 1920), (1, 3, 1920), (1, 2, 0), (1, 2, 2 ** 26 + 1)) + tuple((1, 2, 1920, e) for e in BAD_EDGES):
        assert create(*bad) == fmrx.EINVAL, bad
    assert fmrx.lib.fmrx_audio_spectrum_create(None, 1, 2, 1920, None, 0, 0) == fmrx.EINVAL
    assert fmrx.lib.fmrx_audio_spectrum_destroy(None) == fmrx.OK
    lib = fmrx.lib
    for call in (lambda: lib.fmrx_audio_spectrum_reset(None, 0), lambda: lib.fmrx_audio_spectrum_state_get(None, None),
                 lambda: lib.fmrx_audio_spectrum_process_dev(None, None, 0, 0, None), lambda: lib.fmrx_audio_spectrum_collect(None, None),
                 lambda: lib.fmrx_audio_spectrum_process(None, None, 0, 0, None), lambda: lib.fmrx_audio_spectrum_default_edges(None, None)):
        assert call() == fmrx.EINVAL


def test_8_every_new_symbol_is_exported_and_mirrored(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_audio_spectrum_\w+)\s*\(", text))
    assert declared == {"fmrx_audio_spectrum_" + k for k in ("tables", "frame", "bins", "tile", "max_bands", "default_edges", "walk", "derive", "create",
                                                             "destroy", "reset", "state_get", "process_dev", "collect", "process")}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    for struct, size in (("record", 528), ("state", 2044), ("levels", 544)):
        assert f"sizeof(fmrx_audio_spectrum_{struct}) == {size}" in text
    for name in ("AudioSpectrum", "audioSpectrumWalk", "audioSpectrumDerive", "audioSpectrumTables", "audioSpectrumDefaultEdges", "AUDIO_SPECTRUM_DTYPE",
                 "AUDIO_SPECTRUM_STATE_DTYPE", "AUDIO_SPECTRUM_LEVELS_DTYPE"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_bank", "process_dev", "process", "collect", "state", "reset", "close", "derive", "band_hz"):
        assert hasattr(fmrx.AudioSpectrum, name), name
    assert fmrx.AUDIO_SPECTRUM_DTYPE.itemsize == 528 and fmrx.AUDIO_SPECTRUM_STATE_DTYPE.itemsize == 2044 and fmrx.AUDIO_SPECTRUM_LEVELS_DTYPE.itemsize == 544
    assert fmrx.AUDIO_SPECTRUM_DTYPE == sp.AUDIO_SPECTRUM_DTYPE and fmrx.AUDIO_SPECTRUM_STATE_DTYPE == sp.AUDIO_SPECTRUM_STATE_DTYPE
