"""The true-peak meter without a GPU (include/fmrx.h: fmrx_true_peak_*): the tap table against the
formula, the host walk against the model bit for bit, splits of a row over calls, EBU Tech 3341's true-peak signals, the edge
rules of the levels, the refusals and the exported symbols."""
import re

import numpy as np
import pytest

import _true_peak_model as tp

F32 = np.float32


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_1_the_table_equals_the_formula_and_the_library_equals_the_table(fmrx):
    assert tp.H.shape == (3, 12) and tp.H.dtype == F32
    assert np.array_equal(tp.H.view(np.uint32), tp.formula().view(np.uint32))          # every entry: float32 of the float64 formula
    assert np.array_equal(fmrx.truePeakTaps().view(np.uint32), tp.H.view(np.uint32))
    assert np.array_equal(tp.H[2], tp.H[0][::-1]) and np.array_equal(tp.H[1], tp.H[1][::-1])
    assert [f"{v:08x}" for v in tp.H[0].view(np.uint32)] == tp.H_BITS[0].split()
    assert [f"{v:08x}" for v in tp.H[1, :6].view(np.uint32)] == tp.H_BITS[1].split()
    assert len(np.unique(tp.H)) == 18
    assert fmrx.lib.fmrx_true_peak_latency() == tp.LATENCY == 6 and fmrx.lib.fmrx_true_peak_tile() == 2048
    assert fmrx.TRUE_PEAK_LIMIT == tp.LIMIT == F32(2.0 * 10.0 ** (-1.0 / 20.0)) and fmrx.TRUE_PEAK_CARRY == tp.CARRY == 11


def test_1_no_table_entry_lies_near_a_rounding_midpoint():
    """the float64 value of every entry against the two float32 neighbours' midpoints, in ulps of the entry"""
    j = np.arange(12, dtype=np.float64)
    worst = 1.0
    for p in (1, 2, 3):
        t = (j - 5.0) - p / 4.0
        h = np.sinc(t) * np.i0(5.0 * np.sqrt(1.0 - (t / 6.0) ** 2)) / np.i0(5.0)
        r = h.astype(F32)
        ulp = np.abs(np.nextafter(r, F32(np.inf)).astype(np.float64) - r.astype(np.float64))
        worst = min(worst, float((0.5 - np.abs(h - r.astype(np.float64)) / ulp).min()))
    print(f"the nearest a float64 table value lies to a float32 midpoint: {worst:.3f} ulp")
    assert worst >= 0.09


# ---- the walk -----------------------------------------------------------------------------------------------------------
def host_walk(fmrx, rows, states, limit=tp.LIMIT):
    """fmrx_true_peak_walk channel by channel, in the model's shapes; states float32 [N][2][11] is replaced"""
    rec = np.zeros(rows.shape[0], fmrx.TRUE_PEAK_DTYPE)
    for c in range(rows.shape[0]):
        rec[c], states[c] = fmrx.truePeakWalk(rows[c], states[c], limit)
    return rec


@pytest.mark.parametrize("ac", [1, 2])
@pytest.mark.parametrize("n", [1, 5, 10, 11, 12, 1920])
def test_2_the_host_walk_equals_the_model_bit_for_bit(fmrx, ac, n):
    N = 5
    assert fmrx.TRUE_PEAK_DTYPE == tp.TRUE_PEAK_DTYPE
    rng = np.random.default_rng(100 * ac + n)
    model, states = tp.fresh(N), tp.fresh(N)
    seen = dict(nan=False, inf=False, over=False, within=False)
    for call in range(3):
        x = tp.special_rows(rng, N, ac, n)
        want, model = tp.walk(x, model)
        got = host_walk(fmrx, x, states)
        assert tp.same(got, want), (call, got, want)
        assert tp.same(states[:, :ac], model[:, :ac]) and not states[:, ac:].any(), call
        assert (got["true_peak"] >= got["peak"]).all() and (got["n"] == n).all()
        if ac == 1:
            assert not got["true_peak"][:, 1].any() and not got["peak"][:, 1].any() and not got["over"][:, 1].any()
        seen["inf"] |= bool(np.isinf(want["true_peak"][-1, ac - 1]) and np.isinf(want["peak"][-1, ac - 1]))
        seen["nan"] |= bool(want["over"][-2, 0] > 0 and np.isfinite(want["true_peak"][-2, 0]))
        seen["over"] |= bool(want["over"][:3, :ac].max() > 0)
        seen["within"] |= bool((want["over"][:3, :ac] < n).any())
    assert seen["within"] and (n < 12 or all(seen.values())), seen


def test_2_a_window_with_both_infinities_reads_nan_in_the_phases_and_infinity_from_phase_0(fmrx):
    x = np.zeros((1, 1, 40), F32)
    x[0, 0, 20], x[0, 0, 24] = np.inf, -np.inf
    v = tp.groups(np.concatenate([np.zeros((1, 1, 11), F32), x], axis=2))[0, 0]
    both = [i for i in range(40) if i - 11 <= 20 and 24 <= i]                        # groups whose 12 samples hold both
    # infinity minus infinity where the two taps have one sign (both on one side of the centre), infinity where they differ
    assert np.isnan(v[[24, 25, 30, 31], 1:]).all() and np.isinf(v[[26, 27, 28, 29], 1:]).all() and not np.isfinite(v[both, 1:]).any()
    assert np.isinf(v[20 + 6, 0]) and np.isinf(v[24 + 6, 0]) and np.isfinite(v[:, 0]).sum() == 38
    rec, _ = fmrx.truePeakWalk(x[0])
    want, _ = tp.walk(x, tp.fresh(1))
    assert tp.same(rec, want[0]) and np.isinf(rec["true_peak"][0]) and np.isinf(rec["peak"][0]) and rec["over"][0] == want["over"][0, 0] >= len(both)


def test_2_values_at_the_limit_and_one_ulp_either_side(fmrx):
    """phase 0 alone decides: a lone sample's phases stay below it (every tap is below 1)"""
    for v, over in ((tp.LIMIT, 0), (np.nextafter(tp.LIMIT, F32(0)), 0), (np.nextafter(tp.LIMIT, F32(4)), 1), (-tp.LIMIT, 0),
                    (-np.nextafter(tp.LIMIT, F32(4)), 1)):
        x = np.zeros((1, 30), F32)
        x[0, 10] = v
        rec, _ = fmrx.truePeakWalk(x)
        assert rec["over"][0] == over and rec["true_peak"][0] == rec["peak"][0] == abs(float(v)), (v, rec)
        assert tp.same(rec, tp.walk(x[None], tp.fresh(1))[0][0])


def test_2_denormals_are_kept(fmrx):
    x = np.zeros((1, 40), F32)
    x[0, 12], x[0, 30] = F32(1e-40), F32(-3e-45)
    rec, st = fmrx.truePeakWalk(x)
    want, wst = tp.walk(x[None], tp.fresh(1))
    assert tp.same(rec, want[0]) and tp.same(st[:1], wst[0, :1])
    assert 0 < rec["true_peak"][0] == float(F32(1e-40)) < np.finfo(F32).tiny
    v = tp.groups(np.concatenate([np.zeros(11, F32), x[0]]))
    assert ((v[:, 1:] > 0) & (v[:, 1:] < np.finfo(F32).tiny)).sum() >= 20             # the phases' products are denormal, not zero


def test_3_a_split_over_calls_merges_to_the_one_call_record(fmrx):
    rng = np.random.default_rng(3)
    for ac in (1, 2):
        x = tp.special_rows(rng, 3, ac, 3000)[:1]
        x[0, 0, 999], x[0, ac - 1, 1000] = 2.5, -2.5                                   # peaks whose windows straddle the cuts
        whole, st_w = fmrx.truePeakWalk(x[0])
        st, merged = None, None
        for a, b in ((0, 1000), (1000, 1001), (1001, 3000)):
            rec, st = fmrx.truePeakWalk(x[0][:, a:b], st)
            merged = rec if merged is None else tp.add(merged, rec)
        assert tp.same(merged, whole) and tp.same(st, st_w) and merged["n"] == 3000
        assert tp.same(whole, tp.walk(x, tp.fresh(1))[0][0])


def test_3_a_short_call_shifts_the_state(fmrx):
    x = np.arange(1, 31, dtype=F32).reshape(1, 30)
    st = None
    for a, b in ((0, 4), (4, 5), (5, 15), (15, 30)):
        _, st = fmrx.truePeakWalk(x[:, a:b], st)
        want = np.concatenate([np.zeros(11, F32), x[0, :b]])[-11:]
        assert np.array_equal(st[0], want) and not st[1].any()


# ---- EBU Tech 3341's true-peak signals ----------------------------------------------------------------------------------
def tone(fs_div, phase_deg, amplitude, n=3 * 4800):
    """a sine at fs / fs_div with that start phase and peak amplitude against full scale 2.0, as float32"""
    k = np.arange(n, dtype=np.float64)
    return (tp.FULL_SCALE * amplitude * np.sin(2.0 * np.pi * k / fs_div + np.radians(phase_deg))).astype(F32)


# Tech 3341's cases 15 .. 19: four sines with a peak of 0.50 of full scale (-6.0 dBTP), one whose peak lies 3 dB above full scale;
# name -> fs / f, start phase, amplitude, the level to read, what the model reads in the second and third call
SIGNALS = {"fs/4 at 0 deg": (4, 0.0, 0.5, -6.0, -6.021), "fs/4 at 45 deg": (4, 45.0, 0.5, -6.0, -6.018), "fs/6 at 60 deg": (6, 60.0, 0.5, -6.0, -6.030),
           "fs/8 at 67.5 deg": (8, 67.5, 0.5, -6.0, -6.028), "fs/4 at 45 deg, +3 dB": (4, 45.0, 10.0 ** (3.0 / 20.0), 3.0, 3.003)}


@pytest.mark.parametrize("name", list(SIGNALS))
def test_4_ebu_tech_3341_true_peak_signals(fmrx, name):
    fs_div, phase, amplitude, level, computed = SIGNALS[name]
    x = tone(fs_div, phase, amplitude)
    st, got = None, []
    for c in range(3):
        rec, st = fmrx.truePeakWalk(x[None, 4800 * c:4800 * (c + 1)], st)
        lv = fmrx.truePeakDerive(rec, 1)
        got.append(lv["true_peak_dbtp"][0])
        assert lv["max_dbtp"] == got[-1] and lv["true_peak_dbtp"][1] == -99.0
        if c == 2 and fs_div == 4 and phase == 45.0:
            assert abs(lv["peak_dbfs"][0] - (20.0 * np.log10(amplitude) - 3.0103)) <= 0.001      # what a sample-peak meter reads: 3 dB low
    print(f"{name}: " + ", ".join(f"{v:.3f}" for v in got) + " dBTP in calls 1, 2, 3")
    for v in got[1:]:
        assert -0.4 <= v - level <= 0.2                                                 # Tech 3341's tolerance
        assert abs(v - computed) <= 0.001                                               # the model's figure, to the digits it is quoted in
    assert got[0] >= max(got[1:])                                                       # the abrupt onset reads higher, correctly


# ---- the levels ---------------------------------------------------------------------------------------------------------
def record(**kw):
    r = np.zeros((), tp.TRUE_PEAK_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def levels(fmrx, rec, ac, fs=2.0):
    got, want = fmrx.truePeakDerive(rec, ac, fs), tp.derive(rec, ac, fs)
    flat = dict(true_peak_dbtp_l=got["true_peak_dbtp"][0], true_peak_dbtp_r=got["true_peak_dbtp"][1], peak_dbfs_l=got["peak_dbfs"][0],
                peak_dbfs_r=got["peak_dbfs"][1], max_dbtp=got["max_dbtp"], over_fraction=got["over_fraction"])
    assert set(flat) == set(tp.TRUE_PEAK_LEVELS_NAMES)
    for k in flat:
        assert flat[k] == want[k] or abs(flat[k] - want[k]) <= 1e-12 * abs(want[k]), (k, flat[k], want[k])
    return flat


def test_5_the_levels_and_their_edge_rules(fmrx):
    lv = levels(fmrx, record(n=100, true_peak=(2.0, 1.0), peak=(1.0, 0.5), over=(3, 1)), 2)
    assert lv["true_peak_dbtp_l"] == 0.0 and abs(lv["true_peak_dbtp_r"] - -6.0206) < 1e-4 and abs(lv["peak_dbfs_r"] - -12.0412) < 1e-4
    assert lv["max_dbtp"] == 0.0 and lv["over_fraction"] == 0.02
    mono = levels(fmrx, record(n=100, true_peak=(1.0, 7.0), peak=(1.0, 7.0), over=(4, 0)), 1)      # the second row is not read
    assert mono["true_peak_dbtp_r"] == -99.0 and mono["peak_dbfs_r"] == -99.0 and mono["max_dbtp"] == mono["true_peak_dbtp_l"] and mono["over_fraction"] == 0.04
    zero = levels(fmrx, record(), 2)                                                               # n = 0; dead air reads the floor
    assert zero == dict(true_peak_dbtp_l=-99.0, true_peak_dbtp_r=-99.0, peak_dbfs_l=-99.0, peak_dbfs_r=-99.0, max_dbtp=-99.0, over_fraction=0.0)
    assert levels(fmrx, record(n=1920), 2) == zero
    huge = levels(fmrx, record(n=1, true_peak=(np.inf, 1e30), peak=(np.inf, 1e-30)), 2)
    assert huge["true_peak_dbtp_l"] == 99.0 and huge["true_peak_dbtp_r"] == 99.0 and huge["peak_dbfs_l"] == 99.0 and huge["peak_dbfs_r"] == -99.0
    assert huge["max_dbtp"] == 99.0
    nan = levels(fmrx, record(n=1, true_peak=(np.nan, 1.0), peak=(np.nan, 1.0)), 2)
    assert nan["true_peak_dbtp_l"] == -99.0 and nan["max_dbtp"] == nan["true_peak_dbtp_r"]
    assert levels(fmrx, record(n=10, true_peak=(1.0, 1.0), peak=(1.0, 1.0)), 2, fs=1.0)["max_dbtp"] == 0.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(fmrx.FmrxError):
            fmrx.truePeakDerive(record(), 2, bad)
    with pytest.raises(fmrx.FmrxError):
        fmrx.truePeakDerive(record(), 3)


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_6_refused_and_accepted_parameter_sets(fmrx):
    x, st, rec = np.zeros((2, 16), F32), np.zeros((2, 11), F32), np.zeros(1, fmrx.TRUE_PEAK_DTYPE)
    walk = lambda ac, pitch, n, limit, rows=x.ctypes.data, s=st.ctypes.data, r=rec.ctypes.data: fmrx.lib.fmrx_true_peak_walk(ac, rows, pitch, n, limit, s, r)
    for ok in ((1, 16, 16, 1.0), (2, 16, 16, 1.0), (2, 16, 1, 1e-45), (1, 32, 32, 3e38)):
        assert walk(*ok) == fmrx.OK, ok
    for bad in ((0, 16, 16, 1.0), (3, 16, 16, 1.0), (2, 16, 0, 1.0), (2, 15, 16, 1.0), (2, 16, 16, 0.0), (2, 16, 16, -1.0), (2, 16, 16, float("nan")),
                (2, 16, 16, float("inf")), (1, 2 ** 26 + 1, 2 ** 26 + 1, 1.0)):
        assert walk(*bad) == fmrx.EINVAL, bad
    assert walk(1, 16, 16, 1.0, rows=None) == fmrx.EINVAL and walk(1, 16, 16, 1.0, s=None) == fmrx.EINVAL and walk(1, 16, 16, 1.0, r=None) == fmrx.EINVAL
    h = fmrx.C.c_void_p()
    create = lambda *a: fmrx.lib.fmrx_true_peak_create(fmrx.C.byref(h), *a)
    # parameter sets the create call refuses before it asks for a device
    for bad in ((0, 2, 1920, 1.0, 0), (1, 0, 1920, 1.0, 0), (1, 3, 1920, 1.0, 0), (1, 2, 0, 1.0, 0), (1, 2, 2 ** 26 + 1, 1.0, 0), (1, 2, 1920, 0.0, 0),
                (1, 2, 1920, float("nan"), 0), (1, 2, 1920, float("inf"), 0), (1, 2, 1920, -2.0, 0)):
        assert create(*bad) == fmrx.EINVAL, bad
    assert fmrx.lib.fmrx_true_peak_create(None, 1, 2, 1920, 1.0, 0) == fmrx.EINVAL
    assert fmrx.lib.fmrx_true_peak_destroy(None) == fmrx.OK
    for call in (lambda: fmrx.lib.fmrx_true_peak_reset(None, 0), lambda: fmrx.lib.fmrx_true_peak_state_get(None, None),
                 lambda: fmrx.lib.fmrx_true_peak_process_dev(None, None, 0, 0, None), lambda: fmrx.lib.fmrx_true_peak_collect(None, None),
                 lambda: fmrx.lib.fmrx_true_peak_process(None, None, 0, 0, None)):
        assert call() == fmrx.EINVAL


def test_7_every_new_symbol_is_exported_and_mirrored(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_true_peak_\w+)\s*\(", text))
    assert declared == {"fmrx_true_peak_taps", "fmrx_true_peak_latency", "fmrx_true_peak_tile", "fmrx_true_peak_walk", "fmrx_true_peak_derive",
                        "fmrx_true_peak_create", "fmrx_true_peak_destroy", "fmrx_true_peak_reset", "fmrx_true_peak_state_get",
                        "fmrx_true_peak_process_dev", "fmrx_true_peak_collect", "fmrx_true_peak_process"}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    assert "sizeof(fmrx_true_peak_record) == 56" in text
    for name in ("TruePeak", "truePeakWalk", "truePeakDerive", "truePeakTaps", "TRUE_PEAK_DTYPE", "TRUE_PEAK_LEVELS_DTYPE", "TRUE_PEAK_LIMIT"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_bank", "process_dev", "process", "collect", "state", "reset", "close", "derive"):
        assert hasattr(fmrx.TruePeak, name), name
    assert fmrx.TRUE_PEAK_DTYPE.itemsize == 56 and fmrx.TRUE_PEAK_LEVELS_DTYPE.itemsize == 48
    assert fmrx.TRUE_PEAK_DTYPE == tp.TRUE_PEAK_DTYPE
