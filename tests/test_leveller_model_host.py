"""The loudness leveller / peak limiter's definition (tests/_leveller_model.py) against the host-only part of the C ABI
(fmrx_leveller_control, fmrx_leveller_walk, fmrx_leveller_defaults, parameter validation) and its own stated properties.  No
GPU involved."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _leveller_model as lm

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAM_SETS = {"defaults": {}, "limiter only": dict(max_boost_db=0.0, max_cut_db=0.0),
              "fast, mono scale": dict(attack=1.0, release=0.5, full_scale=1.0, ceiling_dbfs=-0.1, target_lkfs=-16.0, gate_lkfs=-40.0),
              "narrow": dict(max_boost_db=3.0, max_cut_db=1.5, ceiling_dbfs=-6.0)}


def bits_equal(a, b, names=lm.STATUS_DTYPE.names):
    """field for field: the same bits, or both NaN"""
    for k in names:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            ok = (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert np.all(ok), (k, a[k], b[k])


def test_struct_sizes_and_exported_symbols(fmrx):
    assert C.sizeof(fmrx.LevellerParams) == 64 and fmrx.LEVELLER_STATUS_DTYPE.itemsize == 48 and fmrx.LEVELLER_LEVELS_DTYPE.itemsize == 24
    assert fmrx.LEVELLER_STATUS_DTYPE == lm.STATUS_DTYPE and fmrx.AUDIO_METER_DTYPE == lm.AUDIO_METER_DTYPE
    names = ("defaults", "control", "ceiling", "derive", "tile", "walk", "create", "destroy", "reset", "latency", "process_dev", "process",
             "status_get")
    with open(fmrx.HEADER_PATH) as f:
        declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_leveller_\w+)\s*\(", f.read()))
    assert declared == {f"fmrx_leveller_{n}" for n in names}
    for n in declared:
        assert hasattr(fmrx.lib, n), n
    for n in ("Leveller", "LevellerParams", "levellerControl", "levellerWalk", "levellerCeiling", "levellerTile", "levellerDerive",
              "LEVELLER_STATUS_DTYPE", "LEVELLER_LEVELS_DTYPE", "LEVELLER_ONE"):
        assert hasattr(fmrx, n), n
    for n in ("for_bank", "process_bank", "process_dev", "process", "status", "reset", "close", "derive"):
        assert hasattr(fmrx.Leveller, n), n
    header = open(os.path.join(ROOT, "include", "fmrx.h")).read()
    assert "sizeof(fmrx_leveller_status) == 48" in header and "sizeof(fmrx_leveller_params) == 64" in header
    p = fmrx.LevellerParams()
    assert {k: getattr(p, k) for k in lm.PARAM_NAMES} == lm.DEFAULTS
    assert fmrx.LEVELLER_ONE == lm.ONE
    for W in lm.LOOKAHEADS:
        assert fmrx.levellerTile(W) == 2048 - 2 * W
    for W in (0, 4, 7, 12, 96, 256, -64):
        assert fmrx.levellerTile(W) == 0


BAD_PARAMS = [dict(target_lkfs=math.nan), dict(max_boost_db=math.inf), dict(max_cut_db=-math.inf), dict(gate_lkfs=math.nan), dict(attack=math.nan),
              dict(release=math.inf), dict(ceiling_dbfs=math.nan), dict(full_scale=math.inf),
              dict(max_boost_db=-0.5), dict(max_cut_db=-1.0), dict(gate_lkfs=-23.0), dict(gate_lkfs=-10.0), dict(attack=0.0), dict(attack=1.5),
              dict(release=0.0), dict(release=-0.1), dict(release=1.0000001), dict(ceiling_dbfs=0.0), dict(ceiling_dbfs=3.0), dict(full_scale=0.0),
              dict(full_scale=-2.0), dict(target_lkfs=4000.0), dict(gate_lkfs=-4000.0), dict(max_boost_db=7000.0), dict(max_cut_db=7000.0),
              dict(ceiling_dbfs=-800.0), dict(full_scale=1e-30, ceiling_dbfs=-200.0), dict(full_scale=1e200)]
GOOD_PARAMS = [dict(), dict(max_boost_db=0.0, max_cut_db=0.0), dict(attack=1.0, release=1.0), dict(ceiling_dbfs=-1e-9), dict(full_scale=1.0),
               dict(gate_lkfs=-23.000001), dict(ceiling_dbfs=-700.0), dict(full_scale=1e-30)]


def test_parameter_refusals(fmrx):
    st = lm.fresh()
    for kw in BAD_PARAMS:
        assert not lm.valid(lm.params(**kw)), kw
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.levellerControl(fmrx.LevellerParams(**kw), lm.rec(), st)
        assert e.value.code == fmrx.EINVAL, kw
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.levellerCeiling(fmrx.LevellerParams(**kw))
        assert e.value.code == fmrx.EINVAL, kw
    for kw in GOOD_PARAMS:
        assert lm.valid(lm.params(**kw)), kw
        fmrx.levellerControl(fmrx.LevellerParams(**kw), lm.rec(), st)
        assert fmrx.levellerCeiling(fmrx.LevellerParams(**kw)).view(np.uint32) == lm.control(lm.params(**kw))["ceiling"].view(np.uint32)
    for ac in (0, 3):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.levellerControl(None, lm.rec(), st, audio_channels=ac)
        assert e.value.code == fmrx.EINVAL
    x = np.zeros((2, 16), F32)
    for bad in (lambda: fmrx.levellerWalk(x, lookahead=12), lambda: fmrx.levellerWalk(x, lookahead=4), lambda: fmrx.levellerWalk(x, lookahead=256),
                lambda: fmrx.levellerWalk(x, ceiling=0.0), lambda: fmrx.levellerWalk(x, ceiling=math.nan), lambda: fmrx.levellerWalk(x, ceiling=math.inf),
                lambda: fmrx.levellerWalk(np.zeros((2, 0), F32)), lambda: fmrx.levellerWalk(np.zeros((3, 8), F32))):
        with pytest.raises(fmrx.FmrxError) as e:
            bad()
        assert e.value.code == fmrx.EINVAL


def sequences(c, ac):
    def r(lkfs, n=1920):
        return lm.rec_for(c, lkfs, n, ac)
    sub = 5e-324
    return {
        "first call, then louder and quieter": [r(-30), r(-12), r(-12), r(-35), r(-35), r(-23)],
        "gated before the first estimate": [r(-70), lm.rec(1920, (0.0, 0.0)), r(-20), r(-80), r(-20)],
        "NaN, zero and infinite sums": [r(-20), lm.rec(1920, (math.nan, 1.0)), lm.rec(1920, (0.0, 0.0)), lm.rec(1920, (math.inf, 1.0)),
                                        lm.rec(1920, (1.0, math.nan)), lm.rec(1920, (-1.0, -1.0)), lm.rec(0, (0.0, 0.0)), lm.rec(0, (3.0, 3.0)), r(-25),
                                        lm.rec(1920, (sub, sub))],
        "attack": [r(-40)] + [r(-10)] * 12,
        "release": [r(-10)] + [r(-40)] * 12,
        "the boost clamp": [r(-49)] * 3 + [r(-23)] * 3,
        "the cut clamp": [r(5)] * 3 + [r(-23)],
        "enormous and tiny sums": [lm.rec(1920, (1e300, 1e300)), lm.rec(1, (1e-300, 0.0)), r(-23), lm.rec(2 ** 40, (1e9, 1e9))],
        "other lengths": [r(-20, 1), r(-26, 5), r(-18, 4800), r(-30, 1919)],
    }


@pytest.mark.parametrize("ac", [1, 2])
@pytest.mark.parametrize("pset", list(PARAM_SETS))
def test_control_equals_the_model_over_sequences(fmrx, pset, ac):
    p = lm.params(**PARAM_SETS[pset])
    c = lm.control(p)
    lp = fmrx.LevellerParams(**p)
    seen = dict(gated=0, ungated=0, g_min=0, g_max=0, inside=0, moved=0)
    for name, seq in sequences(c, ac).items():
        got = want = lm.fresh()
        for k, r in enumerate(seq):
            got, want = fmrx.levellerControl(lp, r, got, audio_channels=ac), lm.step(c, ac, r, want)
            bits_equal(got, want)
            assert want["calls"] == k + 1 and want["min_code"] == lm.ONE and want["limited"] == 0
            assert c["g_min"] <= want["gain"] <= c["g_max"]
            seen["gated" if want["gated"] else "ungated"] += 1
            seen["g_min" if want["gain"] == c["g_min"] else ("g_max" if want["gain"] == c["g_max"] else "inside")] += 1
            seen["moved"] += int(want["gain0"] != want["gain1"])
    assert seen["gated"] and seen["ungated"] and seen["g_min"]
    if pset == "limiter only":                     # both clamps are 1
        assert not (seen["g_max"] or seen["inside"] or seen["moved"])
    else:
        assert seen["g_max"] and seen["inside"] and seen["moved"]


def test_what_the_control_step_does():
    """the properties the definition states, on the model"""
    c = lm.control(lm.params())
    s = lm.step(c, 2, lm.rec_for(c, -70.0), lm.fresh())                           # under the gate from the start: no estimate, gain 1
    assert s["gated"] == 1 and s["loud_ms"] == 0.0 and s["gain"] == 1.0 and s["gain0"] == 1.0 and s["gain1"] == 1.0
    s = lm.step(c, 2, lm.rec_for(c, -29.0), s)                                    # the first ungated call sets the estimate
    assert s["gated"] == 0 and abs(-0.691 + 10 * math.log10(s["loud_ms"]) + 29.0) < 1e-9
    assert abs(20 * math.log10(s["gain"]) - 6.0) < 1e-4 and s["gain0"] == F32(1.0) and s["gain1"] == F32(s["gain"])
    loud = s["loud_ms"]
    t = lm.step(c, 2, lm.rec_for(c, -80.0), s)                                    # dead air: the estimate and the gain stand
    assert t["gated"] == 1 and t["loud_ms"] == loud and t["gain"] == s["gain"] and t["gain0"] == t["gain1"] == s["gain1"]
    t = lm.step(c, 2, lm.rec_for(c, -19.0), s)                                    # louder: attack 0.2 of the way, in the mean square
    up = lm.rec_for(c, -19.0)["sum_k2"].sum() / 1920 / c["fs2"]
    assert t["loud_ms"] == loud + 0.2 * (up - loud)
    t = lm.step(c, 2, lm.rec_for(c, -39.0), s)                                    # quieter: release 0.02
    dn = lm.rec_for(c, -39.0)["sum_k2"].sum() / 1920 / c["fs2"]
    assert t["loud_ms"] == loud + 0.02 * (dn - loud)
    m = lm.step(c, 1, lm.rec_for(c, -29.0), lm.fresh())                           # a mono channel does not read the second sum
    assert m["loud_ms"] == 0.75 * s["loud_ms"] or abs(m["loud_ms"] / s["loud_ms"] - 0.75) < 1e-12
    lo = lm.control(lm.params(max_boost_db=0.0, max_cut_db=0.0))
    for lkfs in (-45.0, -23.0, 0.0):
        assert lm.step(lo, 2, lm.rec_for(lo, lkfs), lm.fresh())["gain1"] == F32(1.0)


# the bound of test_heron2: four times the worst relative error this grid measured, 1.502e-6 at r = 2^-59 (printed by the
# test).  Two Heron steps from a seed within e0 leave about e0^4 / 8, so the seed is within 5.9 %.
HERON2_BOUND = 4 * 1.502e-6


def test_heron2_against_sqrt():
    worst, at = 0.0, None
    grid = np.concatenate([np.exp(np.linspace(-40.0, 40.0, 160001)), 2.0 ** np.arange(-60, 61), np.linspace(1.0, 4.0, 20001)])
    for r in grid:
        r = float(r)
        e = abs(lm.heron2(r) / math.sqrt(r) - 1.0)
        if e > worst:
            worst, at = e, r
    print(f"heron2: worst relative error {worst:.3e} ({20 * math.log10(1 + worst):.2e} dB) at r = {at!r} over {len(grid)} values of r in e^-40 .. e^40")
    assert worst <= HERON2_BOUND
    for r in (5e-324, 1e-310, 2.2250738585072014e-308, 1.7976931348623157e308):              # the ends of the doubles
        assert abs(lm.heron2(r) / math.sqrt(r) - 1.0) <= HERON2_BOUND, r


def burst_rows(rng, ac, n, W, scale=0.3):
    return lm.special_rows(rng, ac, n, W, max(n // 2, 1), scale)


def same_state(a, b):
    return np.array_equal(a[0], b["codes"]) and np.array_equal(a[1].view(np.uint32), b["u"].view(np.uint32))


def call_lengths(W):
    return [[1], [5], [W - 2], [W - 1], [W], [2 * W - 2], [2 * W - 1], [3 * W + 5, 1, 2 * W + 9], [1, 1, 1, 2, 700]]


@pytest.mark.parametrize("ac", [1, 2])
@pytest.mark.parametrize("W", [8, 64, 128])
def test_walk_equals_the_model(fmrx, W, ac):
    """every call length at which the carried state is cut another way, each as three successive calls (and the sequences of
    unequal calls), on rows with samples beyond the ceiling, a NaN and an infinity"""
    ceiling = lm.control(lm.params())["ceiling"]
    rng = np.random.default_rng(1000 * W + ac)
    limited = nonfinite = 0
    for lengths in call_lengths(W):
        lengths = lengths * 3 if len(lengths) == 1 else lengths
        got_state, want_state = None, lm.fresh_state(ac, W)
        gains = [F32(1.0)] + [F32(g) for g in rng.uniform(0.3, 3.0, len(lengths))]
        for k, n in enumerate(lengths):
            x = burst_rows(rng, ac, n, W, scale=0.8)
            if n >= 5:
                x[rng.integers(ac), rng.integers(n)] = F32([np.nan, np.inf, -np.inf, 7.5][k % 4])
            got, got_state, mn, cnt = fmrx.levellerWalk(x, gains[k], gains[k + 1], W, ceiling, got_state)
            want, want_state, wmn, wcnt = lm.walk(x, gains[k], gains[k + 1], W, ceiling, want_state)
            assert lm.same(got, want).all(), (lengths, k)
            assert same_state(got_state, want_state) and (mn, cnt) == (wmn, wcnt), (lengths, k)
            fin = np.isfinite(want)
            assert np.all(np.abs(want[fin].astype(np.float64)) <= float(ceiling) * (1 + 2.0 ** -22))
            limited += wcnt
            nonfinite += int((~fin).sum())
    assert limited > 0 and nonfinite > 0


@pytest.mark.parametrize("W", [16, 64, 128])
def test_the_bound_holds_on_loud_rows(W):
    """|y| <= c (1 + 2^-22) on every finite output: rows ten times over the ceiling, steps, lone spikes, values next to the
    ceiling on both sides, with and without a gain ramp"""
    c = lm.control(lm.params())["ceiling"]
    rng = np.random.default_rng(W)
    n = 6000
    x = (rng.standard_normal((2, n)) * 6.0).astype(F32)
    x[0, 1000:1400] = F32(17.0)
    x[1, 2000:2600] = F32(1e-3)
    x[:, 2600:3000] = 0.0
    x[0, 2800] = F32(1e30)
    x[1, 3500:3600] = np.nextafter(c, F32(np.inf))
    x[0, 3700:3800] = -c
    x[1, 3900] = F32(3.4e38)
    x[0, 4500] = F32(np.inf)
    for g0, g1 in ((1.0, 1.0), (0.25, 3.98), (3.98, 0.1)):
        state, peak, lim = lm.fresh_state(2, W), 0.0, 0
        for lo in range(0, n, 1500):
            y, state, mn, cnt = lm.walk(x[:, lo:lo + 1500], g0, g1, W, c, state)
            fin = np.isfinite(y)
            peak = max(peak, float(np.abs(y[fin]).max()))
            lim += cnt
        print(f"W {W}, gain {g0} -> {g1}: largest finite |y| / c = 1 + {peak / float(c) - 1:.3e}, {lim} limited outputs")
        assert peak <= float(c) * (1 + 2.0 ** -22) and lim > 0
        assert peak >= float(c) * (1 - 2.0 ** -10)            # and it is a limiter, not a mute: the held peak sits at the ceiling


@pytest.mark.parametrize("W", [8, 64, 128])
def test_unity_gain_and_quiet_input_is_a_pure_delay(fmrx, W):
    c = lm.control(lm.params())["ceiling"]
    rng = np.random.default_rng(5 * W)
    n = 2500
    x = (0.4 * rng.standard_normal((2, n))).astype(F32)
    x[0, 100], x[1, 200], x[0, 300], x[1, 301] = c, -c, F32(-0.0), F32(1e-42)          # at the ceiling is not beyond it
    assert np.abs(x).max() <= c
    want = np.concatenate([np.zeros((2, W - 1), F32), x[:, :n - (W - 1)]], axis=1)
    st_m, st_l, ys_m, ys_l = lm.fresh_state(2, W), None, [], []
    for lo, hi in ((0, 700), (700, 701), (701, n)):
        y, st_m, mn, cnt = lm.walk(x[:, lo:hi], 1.0, 1.0, W, c, st_m)
        assert mn == lm.ONE and cnt == 0
        ys_m.append(y)
        y, st_l, mn, cnt = fmrx.levellerWalk(x[:, lo:hi], 1.0, 1.0, W, c, st_l)
        assert mn == lm.ONE and cnt == 0
        ys_l.append(y)
    for ys in (ys_m, ys_l):
        assert np.array_equal(np.concatenate(ys, axis=1).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("gain", [1.0, 0.37, 2.75])
def test_one_call_equals_three_at_a_fixed_gain(fmrx, gain):
    """3 000 samples in one call and as 1 000 + 1 + 1 999: the same bits, from the model and from the library"""
    W, ac = 64, 2
    c = lm.control(lm.params())["ceiling"]
    x = lm.special_rows(np.random.default_rng(77), ac, 3000, W, 1000, scale=0.9)
    whole, _, mn, cnt = lm.walk(x, gain, gain, W, c, lm.fresh_state(ac, W))
    assert cnt > 0
    st_m, st_l, parts_m, parts_l, cnts = lm.fresh_state(ac, W), None, [], [], 0
    for lo, hi in ((0, 1000), (1000, 1001), (1001, 3000)):
        y, st_m, _, k = lm.walk(x[:, lo:hi], gain, gain, W, c, st_m)
        parts_m.append(y)
        cnts += k
        y, st_l, _, _ = fmrx.levellerWalk(x[:, lo:hi], gain, gain, W, c, st_l)
        parts_l.append(y)
    assert lm.same(np.concatenate(parts_m, axis=1), whole).all() and cnts == cnt
    assert lm.same(np.concatenate(parts_l, axis=1), whole).all()


def test_a_nan_does_not_stay_in_the_state():
    W, ac = 64, 2
    c = lm.control(lm.params())["ceiling"]
    x = (0.3 * np.random.default_rng(3).standard_normal((ac, 1200))).astype(F32)
    x[0, 300], x[1, 600] = np.nan, np.inf
    y, st, mn, cnt = lm.walk(x, 1.0, 1.0, W, c, lm.fresh_state(ac, W))
    d = W - 1
    assert np.isnan(y[0, 300 + d]) and np.isnan(y[1, 600 + d]) and np.isfinite(y[1, 300 + d]) and mn == 0
    bad = ~np.isfinite(y)
    assert bad.sum() == 2 and cnt == 2 * (2 * W - 1)
    assert y[1, 300 + d] == 0.0                                                                                  # the other row, at the NaN: gain 0
    far = np.ones(1200, bool)
    for k in (300, 600):
        far[max(0, k + d - (W - 1)):k + d + W] = False
    far[:d] = False
    assert np.array_equal(y[:, far].view(np.uint32), x[:, np.flatnonzero(far) - d].view(np.uint32))
    y2, st2, mn2, cnt2 = lm.walk(np.full((ac, 500), 0.1, F32), 1.0, 1.0, W, c, st)
    assert np.isfinite(y2).all() and cnt2 == 0 and np.all(st2["codes"] == lm.ONE)


def test_derive(fmrx):
    c = lm.control(lm.params())
    s = lm.step(c, 2, lm.rec_for(c, -29.0), lm.fresh())
    s["min_code"] = lm.ONE // 2
    d = fmrx.levellerDerive(s)
    assert abs(d["loudness_lkfs"] + 29.0) < 1e-9 and abs(d["gain_db"] - 6.0) < 1e-4 and abs(d["reduction_db"] + 6.0206) < 1e-4
    d = fmrx.levellerDerive(lm.fresh())
    assert d["loudness_lkfs"] == -99.0 and d["reduction_db"] == -99.0
