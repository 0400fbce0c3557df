"""The stereo blend / soft mute stage's definition (tests/_blend_model.py) against the host-only part of the C ABI
(fmrx_blend_control, fmrx_blend_defaults, parameter validation), its own stated properties, and the bank capture of the
meters' tests on the CPU models.  No GPU involved."""
import math
import re

import numpy as np
import pytest

import _blend_model as bm
import _meters_model as mm

IF_FS = 240000.0
F32 = np.float32


def bits_equal(a, b, names=bm.STATUS_DTYPE.names):
    """field for field: the same bits, or both NaN"""
    for k in names:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            ok = (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert np.all(ok), (k, a[k], b[k])


def lib_params(fmrx, p):
    return fmrx.BlendParams(**p)


rec, hand_made_records = bm.rec, bm.hand_made_records


PARAM_SETS = bm.PARAM_SETS


@pytest.mark.parametrize("pset", list(PARAM_SETS))
@pytest.mark.parametrize("name", list(hand_made_records()))
def test_control_equals_the_model_on_hand_made_records(fmrx, name, pset):
    """as a first call, and as a second one behind a station's and behind an empty channel's state"""
    p = bm.params(**PARAM_SETS[pset])
    r = hand_made_records()[name]
    for if_Fs in (IF_FS, 250000.0):
        c = bm.control(p, if_Fs)
        starts = [bm.fresh(), bm.step(c, hand_made_records()["a station"], bm.fresh()), bm.step(c, rec((1.0, 1.0, 1.0, 0, 0)), bm.fresh())]
        for st in starts:
            got, want = fmrx.blendControl(lib_params(fmrx, p), if_Fs, r, st), bm.step(c, r, st)
            bits_equal(got, want)


def test_the_edge_rule():
    c = bm.control(bm.params(), IF_FS)
    R = hand_made_records()
    low = ("all zero", "pilot 0", "NaN pilot", "quotient underflows", "infinite both")
    high = ("noise 0, pilot > 0", "NaN noise", "negative noise", "quotient overflows", "infinite pilot", "subnormal noise, ordinary pilot")
    for n in low:
        s = bm.step(c, R[n], bm.fresh())
        assert s["pilot_db"] == -math.inf and s["lamp"] == 0 and s["sep_target"] == 0.0 and s["mono1"] == 1.0, n
    for n in high:
        s = bm.step(c, R[n], bm.fresh())
        assert s["pilot_db"] == math.inf and s["lamp"] == 1 and s["sep_target"] == 1.0 and s["mono1"] == 0.0, n
    s = bm.step(c, R["segments 0"], bm.fresh())
    assert s["quiet_db"] == -math.inf and s["gain_target"] == 0.0 and s["gain1"] == 0.0 and s["lamp"] == 1
    s = bm.step(c, R["all zero"], bm.fresh())
    assert s["quiet_db"] == math.inf and s["gain1"] == 1.0          # ref > 0 over no noise at all: quiet
    s = bm.step(c, R["ordinary noise, subnormal pilot"], bm.fresh())       # a subnormal quotient is a ratio like any other
    assert s["pilot_db"] == (-1072 + 0.75) * bm.DB_PER_OCTAVE and s["lamp"] == 0
    s = bm.step(c, R["subnormal powers"], bm.fresh())
    assert math.isfinite(s["pilot_db"]) and abs(s["pilot_db"] - 10 * math.log10(250.0)) < 0.27


THRESHOLDS = ("pilot_on", "pilot_off", "blend_lo", "blend_hi", "mute_lo", "mute_hi")


@pytest.mark.parametrize("which", THRESHOLDS)
def test_drives_on_a_threshold_and_one_ulp_either_side(fmrx, which):
    """records whose drive is the threshold's pseudo-log2 value exactly, the double below and the double above; from a fresh
    state and from a lit lamp, so that both sides of the hysteresis are crossed"""
    p = bm.params(pilot_on=20.0, pilot_off=14.0, blend_lo=17.0, blend_hi=32.0)       # blend_lo apart from pilot_on
    c = bm.control(p, IF_FS)
    T = p[which] / bm.DB_PER_OCTAVE
    lit = bm.step(c, bm.rec_for(c, 40.0 / bm.DB_PER_OCTAVE, 40.0 / bm.DB_PER_OCTAVE), bm.fresh())
    assert lit["lamp"] == 1
    seen = []
    for d in (math.nextafter(T, -math.inf), T, math.nextafter(T, math.inf)):
        if which.startswith("mute"):
            r = bm.rec_for(c, 40.0 / bm.DB_PER_OCTAVE, d, exact="quiet")
        else:
            r = bm.rec_for(c, d, 40.0 / bm.DB_PER_OCTAVE, exact="pilot")
        for st in (bm.fresh(), lit):
            want = bm.step(c, r, st)
            got = fmrx.blendControl(lib_params(fmrx, p), IF_FS, r, st)
            bits_equal(got, want)
            assert want["quiet_db" if which.startswith("mute") else "pilot_db"] == d * bm.DB_PER_OCTAVE
            seen.append((int(want["lamp"]), float(want["sep_target"]), float(want["gain_target"])))
    fresh_lamps, lit_lamps = [s[0] for s in seen[0::2]], [s[0] for s in seen[1::2]]
    if which == "pilot_on":
        assert fresh_lamps == [0, 1, 1] and lit_lamps == [1, 1, 1]
    if which == "pilot_off":
        assert fresh_lamps == [0, 0, 0] and lit_lamps == [0, 1, 1]
    if which == "blend_lo":
        assert [s[1] for s in seen[1::2]][:2] == [0.0, 0.0] and seen[5][1] > 0.0
    if which == "blend_hi":
        assert seen[1][1] < 1.0 and seen[3][1] == 1.0 and seen[5][1] == 1.0
    if which == "mute_lo":
        assert seen[0][2] == 0.0 and seen[2][2] == 0.0 and seen[4][2] > 0.0
    if which == "mute_hi":
        assert seen[0][2] < 1.0 and seen[2][2] == 1.0 and seen[4][2] == 1.0


sequences = bm.sequences


@pytest.mark.parametrize("pset", list(PARAM_SETS))
@pytest.mark.parametrize("name", ["hysteresis", "attack and release", "mute and recover", "partial", "reset"])
def test_control_equals_the_model_over_call_sequences(fmrx, name, pset):
    p = bm.params(**PARAM_SETS[pset])
    c = bm.control(p, IF_FS)
    got = want = bm.fresh()
    for r in sequences(c)[name]:
        if r is None:
            got = want = bm.fresh()
            continue
        got, want = fmrx.blendControl(lib_params(fmrx, p), IF_FS, r, got), bm.step(c, r, want)
        bits_equal(got, want)


def run(c, recs):
    st, out = bm.fresh(), []
    for r in recs:
        st = bm.fresh() if r is None else bm.step(c, r, st)
        out.append(st)
    return out


def test_what_the_sequences_exercise():
    c = bm.control(bm.params(), IF_FS)
    S = sequences(c)
    assert [int(s["lamp"]) for s in run(c, S["hysteresis"])] == [1, 1, 0, 0, 1]
    s = run(c, S["attack and release"])
    # first call: s = t, no ramp; attack 1: down at once (to the 21 dB target, snapped or not); release 0.25 per call: up in steps
    assert s[0]["sep"] == 1.0 and s[0]["mono0"] == s[0]["mono1"] == 0.0
    assert s[1]["sep"] == s[1]["sep_target"] < 0.1 and s[1]["mono0"] == 0.0 and s[1]["mono1"] > 0.9
    seps = [float(x["sep"]) for x in s[2:]]
    assert seps[0] == s[1]["sep"] + 0.25 * (1.0 - s[1]["sep"])
    assert seps[-1] == 1.0 and s[-1]["mono1"] == 0.0                 # the snap: exactly 1 again, not 1 - 0.75^k
    k = seps.index(1.0)
    assert all(a < b for a, b in zip(seps[:k], seps[1:k + 1])) and all(x == 1.0 for x in seps[k:])
    assert 1.0 - seps[k - 1] > bm.SNAP and 0.75 * (1.0 - seps[k - 1]) <= bm.SNAP
    assert k + 1 == 24                                                # release calls after the fall: 0.97 * 0.75^24 <= 2^-10
    assert all(x["mono0"] == y["mono1"] and x["gain0"] == y["gain1"] for x, y in zip(s[1:], s))   # ramps join across calls
    g = run(c, S["mute and recover"])
    assert g[1]["gain"] == 0.0 and g[1]["gain0"] == 1.0 and g[1]["gain1"] == 0.0 and g[-1]["gain"] == 1.0
    r = run(c, S["reset"])
    assert r[3]["calls"] == 1 and r[3]["mono0"] == r[3]["mono1"] == 0.0 and r[6]["calls"] == 1 and r[6]["gain0"] == r[6]["gain1"] == 0.0
    assert all(0.0 < x["sep_target"] < 1.0 and 0.0 < x["gain_target"] < 1.0 for x in run(c, S["partial"]))


def test_plog2_against_log2():
    for e in list(range(-1074, 1024, 7)) + [-1074, -1022, -1, 0, 1, 1023]:
        assert bm.plog2(math.ldexp(1.0, e)) == float(e)
    rng = np.random.default_rng(20261019)
    r = np.exp2(rng.uniform(-1070.0, 1023.0, 100000))
    err = np.array([math.log2(x) - bm.plog2(x) for x in r])
    print(f"log2 - plog2 over 1e5 doubles: min {err.min():.5f}, max {err.max():.5f}")
    assert err.min() >= -1e-12 and err.max() <= bm.PLOG2_ERROR
    assert bm.PLOG2_ERROR * bm.DB_PER_OCTAVE <= 0.26


def test_parameter_validation(fmrx):
    bad = [dict(blend_hi=20.0), dict(blend_hi=19.0), dict(mute_hi=10.0), dict(mute_lo=30.0), dict(pilot_on=13.0), dict(mute_floor=-0.01),
           dict(mute_floor=1.01), dict(attack=0.0), dict(attack=1.01), dict(release=0.0), dict(release=-1.0), dict(release=2.0),
           dict(pilot_on=math.nan), dict(mute_floor=math.nan), dict(attack=math.nan), dict(blend_hi=math.inf)]
    good = [dict(), dict(pilot_on=14.0), dict(mute_floor=0.0), dict(mute_floor=1.0), dict(attack=1.0, release=1.0), dict(attack=1e-9)]
    r = rec((2e-3, 4e-3, 50.0, 0, 0))
    for kw in bad:
        assert not bm.valid(bm.params(**kw), IF_FS), kw
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.blendControl(fmrx.BlendParams(**kw), IF_FS, r)
        assert e.value.code == fmrx.EINVAL, kw
        if fmrx.device_count() > 0:
            with pytest.raises(fmrx.FmrxError) as e:
                fmrx.Blend(IF_FS, 1, 2, 4, fmrx.BlendParams(**kw))
            assert e.value.code == fmrx.EINVAL, kw
    for kw in good:
        assert bm.valid(bm.params(**kw), IF_FS), kw
        fmrx.blendControl(fmrx.BlendParams(**kw), IF_FS, r)
    for if_Fs in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(fmrx.FmrxError):
            fmrx.blendControl(None, if_Fs, r)


def test_defaults_and_layouts(fmrx):
    p = fmrx.BlendParams()
    assert {k: getattr(p, k) for k in bm.PARAM_NAMES} == bm.DEFAULTS
    assert [n for n, _ in fmrx.BlendParams._fields_] == list(bm.PARAM_NAMES)
    assert fmrx.BLEND_STATUS_DTYPE == bm.STATUS_DTYPE
    assert fmrx.Blend.coef(0.5, 0.04) == 1.0 - math.exp(-0.04 / 0.5)


def test_every_new_symbol_is_exported(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        declared = set(re.findall(r"FMRX_API\s+int\s+(fmrx_blend_\w+)\s*\(", f.read()))
    assert declared == {"fmrx_blend_defaults", "fmrx_blend_control", "fmrx_blend_create", "fmrx_blend_destroy", "fmrx_blend_reset",
                        "fmrx_blend_process_dev", "fmrx_blend_process", "fmrx_blend_status_get"}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    for name in ("BlendParams", "BLEND_STATUS_DTYPE", "blendControl", "Blend"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_bank", "process", "status", "reset", "close", "coef"):
        assert hasattr(fmrx.Blend, name), name


random_rows = bm.random_rows


def test_full_separation_and_full_gain_return_the_input_bits():
    rng = np.random.default_rng(5)
    x = random_rows(rng, 3, 2, 4096)
    assert np.signbit(x[x == 0]).any() and np.isnan(x).any() and np.isinf(x).any()
    y = bm.apply_gains(F32(0), F32(1), x)
    assert bm.same(x, y).all()
    assert np.array_equal(np.signbit(x[x == 0]), np.signbit(y[x == 0]))
    st = bm.step(bm.control(bm.params(), IF_FS), hand_made_records()["noise 0, pilot > 0"], bm.fresh())
    assert st["mono0"] == st["mono1"] == 0.0 and st["gain0"] == st["gain1"] == 1.0
    assert bm.same(x[:1], bm.apply(np.array([st]), x[:1])).all()
    m = random_rows(rng, 2, 1, 1000)
    assert bm.same(m, bm.apply_gains(F32(0), F32(1), m)).all()


def ulp_at(v):
    return np.spacing(np.abs(np.asarray(v, F32)))


def test_full_blend_leaves_left_and_right_one_ulp_apart():
    """a = 1.  The exact values L - D and R + D differ by the rounding error of L - R alone (D = RN(L - R) / 2 exactly), which is
    at most half an ulp of L - R: where L - R is exact (always, by Sterbenz, for L / 2 <= R <= 2 L) L' == R' bit for bit; where
    it is not, the two differ by that error, which is an ulp at the SCALE OF THE INPUT, not of the outputs' own magnitude:
    L = 1 + 2^-23, R = -1 gives L - R = 2 + 2^-23 -> 2, D = 1, L' = 2^-23, R' = 0.  So the ulp of the rule is that of the
    larger of |L| and |R|: |L' - R'| <= ulp(max(|L|, |R|)), measured here: the largest is printed.  The counter-example is
    asserted too, so that nobody reads the rule as one of the outputs' own last places."""
    rng = np.random.default_rng(6)
    x = (0.4 * rng.standard_normal((4, 2, 65536))).astype(F32)
    y = bm.apply_gains(F32(1), F32(1), x)
    big = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))
    d = np.abs(y[:, 0].astype(np.float64) - y[:, 1].astype(np.float64)) / ulp_at(big)
    exact = (x[:, 0].astype(np.float64) - x[:, 1]).astype(F32).astype(np.float64) == x[:, 0].astype(np.float64) - x[:, 1]
    print(f"a = 1: largest |L' - R'| = {d.max():.3f} ulp of max(|L|, |R|); L - R exact in {exact.mean():.3f} of the samples")
    assert d.max() <= 1.0
    assert np.array_equal(y[:, 0][exact].view(np.uint32), y[:, 1][exact].view(np.uint32))
    mono = (x[:, 0].astype(np.float64) + x[:, 1]) / 2
    e = np.abs(y.astype(np.float64) - mono[:, None, :]).max(axis=1) / ulp_at(big)
    print(f"a = 1: largest distance from (L + R) / 2 = {e.max():.3f} ulp of max(|L|, |R|)")
    assert e.max() <= 1.0
    cx = np.array([[[1.0 + 2.0 ** -23], [-1.0]]], F32)
    cy = bm.apply_gains(F32(1), F32(1), cx)
    assert cy[0, 0, 0] == F32(2.0 ** -23) and cy[0, 1, 0] == 0.0


def test_ramps():
    a = bm.ramps([0.0, 1.0, 0.25, 0.5], [1.0, 0.0, 0.25, 0.5000001], 1920)
    assert a.dtype == F32 and a.shape == (4, 1920)
    assert a[0, -1] == 1.0 and a[1, -1] == 0.0 and np.all(a[2] == F32(0.25))
    assert np.all(np.diff(a[0]) >= 0) and np.all(np.diff(a[1]) <= 0) and a.min() >= 0.0 and a.max() <= 1.0
    assert abs(float(a[0, 959]) - 0.5) < 1e-6
    for n in (1, 4, 5, 1020, 1923):
        r = bm.ramps([0.0, 1.0], [1.0, 0.0], n)
        assert abs(float(r[0, -1]) - 1.0) <= 2.0 ** -22 and abs(float(r[1, -1])) <= 2.0 ** -22   # n * float32(1 / n) is 1 to within an ulp or two


def test_the_bank_capture_meets_its_conditions_on_the_cpu_models(oracle):
    """The chain of test_meters_model_host.py::test_the_bank_capture_meets_its_conditions_on_the_cpu_models with the blend's
    control step behind it, default parameters.  On all three calls channels 0-3 (the stations, one mistuned) read lamp on,
    separation 1 and gain 1; channels 4-7 (empty) read lamp off, separation 0 and gain = floor.  Measured on these models,
    over the three calls, in pseudo-dB (plog2 reads up to 0.26 dB below the true ratio; true dB in brackets): the stations' pilot
    ratio is at least 38.39 (38.56) against blend_hi 32, their quieting at least 45.58 (45.73) against mute_hi 24; the empty
    channels' pilot ratio is at most 1.42 (1.68) against pilot_on 20, their quieting at most 2.52 (2.64) against mute_lo 10: the
    smallest margin is 6.4 dB, against 0.26 dB of plog2 error."""
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
    p = bm.params()
    c = bm.control(p, IF_FS)
    state = bm.fresh(8)
    worst = dict(sp=math.inf, sq=math.inf, ep=-math.inf, eq=-math.inf)
    for i in range(MC.CALLS):
        tuned = model.process(wide[2 * n_wide * i:2 * n_wide * (i + 1)])
        recs = [mm.record(tuned[k], pipes[k].process(tuned[k])["demod"], IF_FS) for k in range(8)]
        state = bm.step_all(c, recs, state)
        for k in range(4):
            assert state[k]["lamp"] == 1 and state[k]["sep"] == 1.0 and state[k]["gain"] == 1.0, (i, k)
            assert state[k]["mono0"] == state[k]["mono1"] == 0.0 and state[k]["gain0"] == state[k]["gain1"] == 1.0, (i, k)
        for k in range(4, 8):
            assert state[k]["lamp"] == 0 and state[k]["sep"] == 0.0 and state[k]["gain"] == p["mute_floor"], (i, k)
            assert state[k]["mono0"] == state[k]["mono1"] == 1.0 and state[k]["gain1"] == 0.0, (i, k)
        worst["sp"] = min(worst["sp"], state["pilot_db"][:4].min())
        worst["sq"] = min(worst["sq"], state["quiet_db"][:4].min())
        worst["ep"] = max(worst["ep"], state["pilot_db"][4:].max())
        worst["eq"] = max(worst["eq"], state["quiet_db"][4:].max())
    print("pseudo-dB over the three calls: stations' pilot ratio >= {sp:.2f}, quieting >= {sq:.2f}; empty channels' pilot ratio <= {ep:.2f}, "
          "quieting <= {eq:.2f}".format(**worst))
    margins = (worst["sp"] - p["blend_hi"], worst["sq"] - p["mute_hi"], p["pilot_on"] - worst["ep"], p["mute_lo"] - worst["eq"])
    assert min(margins) > bm.PLOG2_ERROR * bm.DB_PER_OCTAVE      # no decision within plog2's error of its threshold
