"""The variable high-cut stage's definition (tests/_highcut_model.py) against the host-only part of the C ABI
(fmrx_highcut_design, fmrx_highcut_control, fmrx_highcut_defaults, parameter validation), its own stated properties -- the
parallel walk returns the serial walk's bits, identity at cut 0, DC gain 1, the one-pole response -- and the bank capture of
the meters' tests on the CPU models.  No GPU involved."""
import math
import re

import numpy as np
import pytest

import _highcut_model as hm
import _meters_model as mm

IF_FS, AUDIO_FS = 240000.0, 48000.0
F32 = np.float32


def bits_equal(a, b, names=hm.STATUS_DTYPE.names):
    """field for field: the same bits, or both NaN"""
    for k in names:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            ok = (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert np.all(ok), (k, a[k], b[k])


def test_design_values_and_refusals(fmrx):
    p_max_d, p_max = hm.design(2500.0, AUDIO_FS)
    assert p_max_d == math.exp(-2.0 * math.pi * 2500.0 / AUDIO_FS) and abs(float(p_max) - 0.72090) < 5e-6
    assert fmrx.highCutDesign(2500.0, AUDIO_FS).view(np.uint32) == p_max.view(np.uint32)
    # the pole moves linearly with the cut: half cut and full cut at 48 kHz, the figures of DESIGN.md 4.13
    half, full = float(p_max) / 2, float(p_max)
    db = lambda g: 20.0 * math.log10(g)
    # (figures quoted to a tenth of a dB: within a tenth; the exact ones are -1.35, -5.41, -6.83 and -14.25 dB)
    assert abs(db(hm.response(half, 5e3, AUDIO_FS)) + 1.35) < 0.01 and abs(db(hm.response(half, 15e3, AUDIO_FS)) + 5.4) < 0.1
    assert abs(db(hm.response(full, 5e3, AUDIO_FS)) + 6.8) < 0.1 and abs(db(hm.response(full, 15e3, AUDIO_FS)) + 14.3) < 0.1
    assert abs(db(hm.response(full, 2500.0, AUDIO_FS)) + 3.0) < 0.1               # the corner at full cut is fc_min
    for fc in (0.0, -1.0, -2500.0, math.nan, math.inf):
        assert hm.design(fc, AUDIO_FS) is None
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.highCutDesign(fc, AUDIO_FS)
        assert e.value.code == fmrx.EINVAL
        with pytest.raises(fmrx.FmrxError):
            fmrx.highCutControl(fmrx.HighCutParams(fc_min=fc), IF_FS, AUDIO_FS, hm.rec())
    for fs in (0.0, -48000.0, math.nan, math.inf):
        assert hm.design(2500.0, fs) is None
        with pytest.raises(fmrx.FmrxError):
            fmrx.highCutDesign(2500.0, fs)
    # the cap: walk the doubles around the fc_min whose float32 pole is 0.875 exactly
    fc = -math.log(0.875) * AUDIO_FS / (2.0 * math.pi)
    while hm.design(fc, AUDIO_FS) is not None:           # down until refused ...
        fc = math.nextafter(fc, 0.0) - 1e-9
    while hm.design(fc, AUDIO_FS) is None:               # ... and up to the first one accepted
        last_refused, fc = fc, math.nextafter(fc, math.inf)
    assert F32(math.exp(-2.0 * math.pi * last_refused / AUDIO_FS)) > F32(0.875) and hm.design(fc, AUDIO_FS)[1] == F32(0.875)
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.highCutDesign(last_refused, AUDIO_FS)
    assert e.value.code == fmrx.EINVAL
    assert fmrx.highCutDesign(fc, AUDIO_FS) == F32(0.875)
    assert not hm.valid(hm.params(fc_min=last_refused), IF_FS, AUDIO_FS) and hm.valid(hm.params(fc_min=fc), IF_FS, AUDIO_FS)
    with pytest.raises(fmrx.FmrxError):
        fmrx.highCutControl(fmrx.HighCutParams(fc_min=last_refused), IF_FS, AUDIO_FS, hm.rec())
    fmrx.highCutControl(fmrx.HighCutParams(fc_min=fc), IF_FS, AUDIO_FS, hm.rec())


@pytest.mark.parametrize("pset", list(hm.PARAM_SETS))
@pytest.mark.parametrize("name", list(hm.hand_made_records()))
def test_control_equals_the_model_on_hand_made_records(fmrx, name, pset):
    """as a first call, and as a second one behind an open and behind a fully cut channel's state"""
    p = hm.params(**hm.PARAM_SETS[pset])
    r = hm.hand_made_records()[name]
    for if_Fs in (IF_FS, 250000.0):
        c = hm.control(p, if_Fs, AUDIO_FS)
        starts = [hm.fresh(), hm.step(c, hm.hand_made_records()["all zero"], hm.fresh()), hm.step(c, hm.rec((1e6, 1e6, 1.0, 0, 0)), hm.fresh())]
        assert starts[1]["open"] == 1.0 and starts[2]["open"] == 1.0 - p["cut_max"]
        for st in starts:
            got, want = fmrx.highCutControl(fmrx.HighCutParams(**p), if_Fs, AUDIO_FS, r, st), hm.step(c, r, st)
            bits_equal(got, want)


def test_the_edge_rule():
    c = hm.control(hm.params(), IF_FS, AUDIO_FS)
    R = hm.hand_made_records()
    for n in ("all zero", "NaN noise", "negative noise", "subnormal powers"):        # no noise to speak of (or none that counts): open
        s = hm.step(c, R[n], hm.fresh())
        assert s["quiet_db"] == math.inf and s["open"] == 1.0 and s["p0"] == s["p1"] == 0.0, n
    for n in ("segments 0", "infinite noise"):
        s = hm.step(c, R[n], hm.fresh())
        assert s["quiet_db"] == -math.inf and s["open"] == 0.0 and s["p1"] == c["p_max"], n


@pytest.mark.parametrize("which", ["hc_lo", "hc_hi"])
def test_drives_on_a_threshold_and_one_double_either_side(fmrx, which):
    p = hm.params()
    c = hm.control(p, IF_FS, AUDIO_FS)
    T = p[which] / hm.DB_PER_OCTAVE
    cut = hm.step(c, hm.rec_for(c, 40.0 / hm.DB_PER_OCTAVE, 5.0 / hm.DB_PER_OCTAVE), hm.fresh())
    assert cut["open"] == 0.0
    seen = []
    for d in (math.nextafter(T, -math.inf), T, math.nextafter(T, math.inf)):
        r = hm.rec_for(c, 40.0 / hm.DB_PER_OCTAVE, d, exact="quiet")
        for st in (hm.fresh(), cut):
            want = hm.step(c, r, st)
            bits_equal(fmrx.highCutControl(fmrx.HighCutParams(**p), IF_FS, AUDIO_FS, r, st), want)
            assert want["quiet_db"] == d * hm.DB_PER_OCTAVE
            seen.append(float(want["open_target"]))
    if which == "hc_lo":
        assert seen[0] == 0.0 and seen[2] == 0.0 and seen[4] > 0.0
    else:
        # (d - lo) * (1 / (hi - lo)) is two rounded operations: on the threshold itself it may read one double below 1
        assert seen[0] < 1.0 and seen[0] <= seen[2] <= seen[4] == 1.0 and seen[2] >= 1.0 - 2.0 ** -52


@pytest.mark.parametrize("pset", list(hm.PARAM_SETS))
@pytest.mark.parametrize("name", ["walk", "attack and release", "partial", "reset", "full"])
def test_control_equals_the_model_over_call_sequences(fmrx, name, pset):
    p = hm.params(**hm.PARAM_SETS[pset])
    c = hm.control(p, IF_FS, AUDIO_FS)
    got = want = hm.fresh()
    for r in hm.sequences(c)[name]:
        if r is None:
            got = want = hm.fresh()
            continue
        got, want = fmrx.highCutControl(fmrx.HighCutParams(**p), IF_FS, AUDIO_FS, r, got), hm.step(c, r, want)
        bits_equal(got, want)


def run(c, recs):
    st, out = hm.fresh(), []
    for r in recs:
        st = hm.fresh() if r is None else hm.step(c, r, st)
        out.append(st)
    return out


def test_what_the_sequences_exercise():
    c = hm.control(hm.params(), IF_FS, AUDIO_FS)
    S = hm.sequences(c)
    w = run(c, S["walk"])
    assert w[0]["p0"] == w[0]["p1"] == 0.0 and 0.0 < w[1]["p1"] < c["p_max"] and w[2]["p1"] == c["p_max"]       # 0 -> partial -> full
    assert 0.0 < w[3]["p1"] < c["p_max"] and w[-1]["open"] < 1.0                                               # release 0.25: not open again yet
    assert all(x["p0"] == y["p1"] for x, y in zip(w[1:], w))                                                   # ramps join across calls
    s = run(c, S["attack and release"])
    assert s[0]["open"] == 1.0 and s[1]["open"] == s[1]["open_target"] < 0.1                                   # attack 1: down at once
    opens = [float(x["open"]) for x in s[2:]]
    assert opens[0] == s[1]["open"] + 0.25 * (1.0 - s[1]["open"]) and opens[-1] == 1.0 and s[-1]["p1"] == 0.0  # the snap: exactly open again
    k = opens.index(1.0)
    assert 1.0 - opens[k - 1] > hm.bm.SNAP and 0.75 * (1.0 - opens[k - 1]) <= hm.bm.SNAP
    r = run(c, S["reset"])
    assert r[3]["calls"] == 1 and r[3]["p0"] == r[3]["p1"] == 0.0 and r[6]["calls"] == 1 and r[6]["p0"] == r[6]["p1"] == c["p_max"]
    assert all(0.0 < x["open_target"] < 1.0 for x in run(c, S["partial"]))
    h = hm.control(hm.params(cut_max=0.5), IF_FS, AUDIO_FS)
    assert run(h, S["full"])[0]["open"] == 0.5 and run(h, S["full"])[0]["p1"] == F32(0.5 * h["p_max_d"])


def test_parameter_validation(fmrx):
    bad = [dict(hc_hi=16.0), dict(hc_hi=15.0), dict(hc_lo=40.0), dict(cut_max=-0.01), dict(cut_max=1.01), dict(attack=0.0), dict(attack=1.01),
           dict(release=0.0), dict(release=-1.0), dict(release=2.0), dict(hc_lo=math.nan), dict(cut_max=math.nan), dict(attack=math.nan),
           dict(hc_hi=math.inf), dict(fc_min=1000.0), dict(segment=0), dict(segment=-2), dict(warmup=-2), dict(warmup=(1 << 20) + 1)]
    good = [dict(), dict(cut_max=0.0), dict(cut_max=1.0), dict(attack=1.0, release=1.0), dict(attack=1e-9), dict(warmup=0, segment=1),
            dict(warmup=8, segment=16), dict(fc_min=23999.0)]
    r = hm.rec((2e-3, 4e-3, 50.0, 0, 0))
    for kw in bad:
        assert not hm.valid(hm.params(**kw), IF_FS, AUDIO_FS), kw
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.highCutControl(fmrx.HighCutParams(**kw), IF_FS, AUDIO_FS, r)
        assert e.value.code == fmrx.EINVAL, kw
        if fmrx.device_count() > 0:
            with pytest.raises(fmrx.FmrxError) as e:
                fmrx.HighCut(IF_FS, AUDIO_FS, 1, 2, 4, fmrx.HighCutParams(**kw))
            assert e.value.code == fmrx.EINVAL, kw
    for kw in good:
        assert hm.valid(hm.params(**kw), IF_FS, AUDIO_FS), kw
        fmrx.highCutControl(fmrx.HighCutParams(**kw), IF_FS, AUDIO_FS, r)
    for if_Fs in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(fmrx.FmrxError):
            fmrx.highCutControl(None, if_Fs, AUDIO_FS, r)


def test_defaults_and_layouts(fmrx):
    p = fmrx.HighCutParams()
    assert {k: getattr(p, k) for k in hm.PARAM_NAMES} == hm.DEFAULTS
    assert [n for n, _ in fmrx.HighCutParams._fields_] == list(hm.PARAM_NAMES)
    assert fmrx.HIGHCUT_STATUS_DTYPE == hm.STATUS_DTYPE


def test_every_new_symbol_is_exported(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        declared = set(re.findall(r"FMRX_API\s+int\s+(fmrx_highcut_\w+)\s*\(", f.read()))
    assert declared == {"fmrx_highcut_defaults", "fmrx_highcut_design", "fmrx_highcut_control", "fmrx_highcut_create", "fmrx_highcut_destroy",
                        "fmrx_highcut_reset", "fmrx_highcut_set_force", "fmrx_highcut_process_dev", "fmrx_highcut_process",
                        "fmrx_highcut_status_get", "fmrx_highcut_diagnostics"}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    for name in ("HighCutParams", "HIGHCUT_STATUS_DTYPE", "highCutControl", "highCutDesign", "HighCut"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_dev", "process_bank", "process", "status", "reset", "diagnostics", "force_serial", "close"):
        assert hasattr(fmrx.HighCut, name), name


# ---- the walks -------------------------------------------------------------------------------------------------------
P_MAX = hm.design(2500.0, AUDIO_FS)[1]
RAMPS = {"0 -> p_max": (F32(0), P_MAX), "p_max -> 0": (P_MAX, F32(0)), "constant p_max": (P_MAX, P_MAX)}
SHAPES = {"(8, 16)": (8, 16), "(64, 64)": (64, 64), "built-in": (hm.BUILTIN_W, hm.BUILTIN_L)}


@pytest.fixture(scope="module")
def fixed():
    d = hm.fixed_inputs(4096)
    return np.stack([d["audio"], d["audio->silence"], d["impulse"]])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("ramp", list(RAMPS))
def test_parallel_returns_serials_bits_and_state(fixed, ramp, shape):
    """the three fixed inputs as three rows, three calls (1500, 1300 and 1296 samples) with carried state: the ramp, its end
    point held, the ramp back"""
    a, b = RAMPS[ramp]
    W, L = SHAPES[shape]
    ss = sp = None
    at, total = 0, 0
    for n, (p0, p1) in zip((1500, 1300, 1296), ((a, b), (b, b), (b, a))):
        x = fixed[:, at:at + n]
        at += n
        ys, ss = hm.serial(x, p0, p1, P_MAX, ss)
        yp, sp, missed, segs = hm.parallel(x, p0, p1, P_MAX, sp, W, L)
        assert hm.same(ys, yp).all() and hm.same(ss, sp).all(), (ramp, shape)
        assert segs == 3 * ((n + L - 1) // L - 1)
        total += missed
    print(f"{ramp}, {shape}: {total} segments walked again over the three calls")
    assert shape != "(8, 16)" or total > 0


def test_the_small_shape_misses_and_the_builtin_does_not_on_audio(fixed):
    """the first row of DESIGN.md 4.13's table and its hardest one: a pole held at the cap"""
    audio = fixed[0]
    for p0, p1, p_max in ((F32(0), F32(0.72), F32(0.72)), (F32(0.875), F32(0.875), F32(0.875))):
        small = hm.parallel(audio, p0, p1, p_max, None, 8, 16)[2]
        built = hm.parallel(audio, p0, p1, p_max, None, hm.BUILTIN_W, hm.BUILTIN_L)[2]
        print(f"pole {p0} -> {p1} on `audio`: (8, 16) misses {small} of 255 segments, the built-in shape {built} of 15")
        assert small > 0 and built == 0


def test_identity_at_cut_0():
    rng = np.random.default_rng(5)
    x = hm.random_rows(rng, 3, 2, 2048).reshape(6, 2048)
    x[0, :8] = [1e-40, -1e-40, 0.0, -0.0, math.nan, math.inf, -math.inf, 1e-45]
    assert np.signbit(x[x == 0]).any() and np.isnan(x).any() and np.isinf(x).any()
    for walk in (lambda: hm.serial(x, 0.0, 0.0, P_MAX)[0], lambda: hm.parallel(x, 0.0, 0.0, P_MAX, None, 8, 16)[0]):
        y = walk()
        assert hm.same(x, y).all()
        assert np.array_equal(x[~np.isnan(x)].view(np.uint32), y[~np.isnan(x)].view(np.uint32))      # -0 and subnormals with their bits
    # ... and a pole that has come down to 0 forgets an infinite state at once: the select, not fmaf(0, inf, x)
    y = hm.serial(np.array([[math.inf, 1.0, 2.0]], F32), P_MAX, 0.0, P_MAX)[0]
    assert np.isinf(y[0, 0]) and y[0, 2] == 2.0


def test_dc_gain_is_1():
    """q + p is 1 to within half an ulp of q, and the walk of a constant settles where y = fmaf(p, y, q c) maps y to itself:
    within a few ulps of c"""
    for p in (F32(0.1), F32(0.3), P_MAX, F32(0.875)):
        for cst in (F32(1.0), F32(-0.37)):
            y = hm.serial(np.full((1, 600), cst, F32), p, p, F32(0.875))[0]
            assert abs(float(y[0, -1]) - float(cst)) <= 4 * np.spacing(np.abs(cst)), (p, cst, y[0, -1])


@pytest.mark.parametrize("f", [1e3, 5e3, 10e3, 15e3])
def test_steady_state_gain(f):
    """The walk against |(1 - p) / (1 - p e^{-jw})| at a pole held at p.  Tolerance, with u = 2^-24 and an input of amplitude
    A: q = RN(1 - p) is off by at most u q; v = RN(q x) adds u |v| <= u q A; the fused multiply-add rounds once, u |y| <= u A.
    So every step adds at most d = u A (1 + 2 q) to the error e, and e[k] = p e[k-1] + d[k] stays below d / (1 - p) =
    u A (1 / q + 2) <= 10 u A for p <= 0.875 (q >= 0.125).  The gain is read as |Y / X| from the DFT bin of both over whole
    periods (the input is the float32 row itself, so its own rounding cancels), which moves it by at most max |e| / A:
    10 u, to which 2 u are added for the float64 evaluation and the transient left after 528 samples (0.875^528 < 2^-100)."""
    n, skip, A = 4800 + 528, 528, 0.4
    t = np.arange(n)
    x = (A * np.sin(2 * np.pi * f * t / AUDIO_FS + 0.3)).astype(F32)[None, :]
    e = np.exp(-2j * np.pi * f * t[skip:] / AUDIO_FS)
    for p in (F32(0.25), F32(float(P_MAX) / 2), P_MAX, F32(0.875)):
        y = hm.serial(x, p, p, F32(0.875))[0]
        gain = abs(np.dot(y[0, skip:].astype(np.float64), e)) / abs(np.dot(x[0, skip:].astype(np.float64), e))
        want = hm.response(float(p), f, AUDIO_FS)
        print(f"p = {float(p):.5f}, {f / 1e3:.0f} kHz: gain {gain:.8f}, one-pole response {want:.8f}, difference {abs(gain - want) / 2.0 ** -24:.2f} u")
        assert abs(gain - want) <= 12 * 2.0 ** -24


def test_the_bank_capture_meets_its_conditions_on_the_cpu_models(oracle):
    """The chain of test_blend_model_host.py's test of the same name with the high-cut's control step behind it, default
    parameters.  On all three calls channels 0-3 (the stations, one mistuned) read open = 1 and p1 = 0; channels 4-7 (empty)
    read open = 0 and p1 = p_max.  Measured on these models over the three calls, in pseudo-dB: the stations' quieting is at
    least 45.58 against hc_hi 36, the empty channels' at most 2.52 against hc_lo 16: the smallest margin is 9.58 dB, against
    0.26 dB of plog2 error."""
    import _meters_capture as MC
    import _tuner_capture as TC
    import _tuner_model as tm
    cap = TC.RDS
    wide = MC.capture()
    h = oracle.impulse_response_lpf(cap["Fs_w"], cap["cutoff"], cap["T"])
    model = tm.TunerModel(h, cap["R"], 8)
    for k, (f, g) in enumerate(MC.channels()):
        model.set_channel(k, f, cap["Fs_w"], g)
    pipes = [oracle.pipeline(0, 2) for _ in range(8)]
    n_wide = MC.BYTES_PER_CALL // 2 * cap["R"]
    p = hm.params()
    c = hm.control(p, IF_FS, AUDIO_FS)
    state = hm.fresh(8)
    lo, hi = math.inf, -math.inf
    for i in range(MC.CALLS):
        tuned = model.process(wide[2 * n_wide * i:2 * n_wide * (i + 1)])
        recs = [mm.record(tuned[k], pipes[k].process(tuned[k])["demod"], IF_FS) for k in range(8)]
        state = hm.step_all(c, recs, state)
        for k in range(4):
            assert state[k]["open"] == 1.0 and state[k]["p0"] == state[k]["p1"] == 0.0, (i, k)
        for k in range(4, 8):
            assert state[k]["open"] == 0.0 and state[k]["p1"] == c["p_max"], (i, k)
        lo, hi = min(lo, state["quiet_db"][:4].min()), max(hi, state["quiet_db"][4:].max())
    margin = min(lo - p["hc_hi"], p["hc_lo"] - hi)
    print(f"pseudo-dB over the three calls: stations' quieting >= {lo:.2f}, empty channels' <= {hi:.2f}; smallest margin {margin:.2f} dB")
    assert margin > hm.bm.PLOG2_ERROR * hm.DB_PER_OCTAVE
