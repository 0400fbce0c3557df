"""tests/_meters_order_model.py on the CPU: its float64 fma against exact rational arithmetic; the order model against the
meters' definition (tests/_meters_model.py) within that file's bounds, on every row tests/test_gpu_meters_exact.py compares the
device on; and the comparison's power: six deliberate mistakes in the order each change the bits of a compared field on the rows
of every one of that file's tests.  No GPU involved.

Case (d)'s rows are a receiver bank's discriminator rows and exist on a GPU only; here the oracle's discriminator stands in
for them on the same input streams (the GPU test repeats the power check on the rows it gets)."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import _meters_exact_cases as mc
import _meters_model as mm
import _meters_order_model as om

L = mm.SEGMENT


# ---------------------------------------------------------------------------------------------------------------------------
# fma64 against Fraction
# ---------------------------------------------------------------------------------------------------------------------------
def exact_fma(d, t, a) -> float:
    """fma of three finite doubles, rounded once (int / int is correctly rounded in CPython); a zero result by IEEE's rules."""
    r = Fraction(d) * Fraction(t) + Fraction(a)
    if r != 0:
        return float(r)
    p_zero, p_neg = d == 0.0 or t == 0.0, (np.signbit(d) != np.signbit(t))
    if p_zero and a == 0.0 and bool(p_neg) == bool(np.signbit(a)):
        return -0.0 if p_neg else 0.0        # (+-0) + (+-0) of one sign keeps it
    return 0.0                               # x + (-x), and zeros of unlike signs, round to +0


def check_fma(d, t, a, what):
    d, t, a = (np.asarray(v, np.float64).reshape(-1) for v in np.broadcast_arrays(d, t, a))
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64)), "d must hold float32 values"
    got = om.fma64(d, t, a)
    want = np.array([exact_fma(float(x), float(y), float(z)) for x, y, z in zip(d, t, a)])
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    unfused = int(np.count_nonzero((d * t + a).view(np.uint64) != want.view(np.uint64)))
    print(f"{what}: {len(d)} cases, {len(bad)} differ; the unfused d * t + a differs in {unfused}")
    assert len(bad) == 0, f"{what}: first at {bad[0]}: fma({d[bad[0]]!r}, {t[bad[0]]!r}, {a[bad[0]]!r}) = {got[bad[0]]!r}, exact {want[bad[0]]!r}"
    return unfused


def samples(rng, n):
    return (rng.uniform(-1.5, 1.5, n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32).astype(np.float64)


def test_fma_random_operands():
    rng = np.random.default_rng(501)
    n = 20000
    d, t = samples(rng, n), rng.uniform(-1.0, 1.0, n)
    a = d * t * rng.uniform(-4.0, 4.0, n) * 2.0 ** rng.integers(-30, 31, n)
    unfused = check_fma(d, t, a, "random")
    assert unfused > n // 10          # the fma is visible in the bits: the mutant 'unfused' has something to change


def test_fma_cancellation():
    """a = -fl(d t) and its neighbours: the result is the product's rounding error, or that plus an ulp of a"""
    rng = np.random.default_rng(502)
    n = 5000
    d, t = samples(rng, n), rng.uniform(-1.0, 1.0, n)
    p = -(d * t)
    for a, what in ((p, "a = -fl(d t)"), (np.nextafter(p, np.inf), "one ulp above"), (np.nextafter(p, -np.inf), "one ulp below"),
                    (p * (1.0 + rng.uniform(-1e-9, 1e-9, n)), "within 1e-9")):
        check_fma(d, t, a, "cancellation, " + what)


def test_fma_on_and_beside_rounding_ties():
    """a = (2^52 + r) 2^e and d t = q 2^(e-1) with q odd: exactly halfway between two doubles; then t one ulp to either side"""
    rng = np.random.default_rng(503)
    n = 4000
    e = rng.integers(-40, 41, n).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], n)
    a = sign * (2.0 ** 52 + rng.integers(0, 2 ** 51, n).astype(np.float64)) * 2.0 ** e
    d = (2 * rng.integers(0, 2 ** 11, n) + 1).astype(np.float64)                        # odd, 12 bits
    t = rng.choice([-1.0, 1.0], n) * (2 * rng.integers(0, 2 ** 19, n) + 1).astype(np.float64) * 2.0 ** (e - 1.0)
    on = check_fma(d, t, a, "ties")
    assert on == 0                    # on a tie the product is exact, so the unfused form rounds the same exact sum
    # beside it the product has more than 53 bits and its last ones decide the direction: the low part must not be lost
    check_fma(d, np.nextafter(t, np.inf), a, "one ulp of t above a tie")
    check_fma(d, np.nextafter(t, -np.inf), a, "one ulp of t below a tie")
    # and a, not t, moved off the tie
    check_fma(d, t, np.nextafter(a, np.inf), "one ulp of a above a tie")
    check_fma(d, t, np.nextafter(a, -np.inf), "one ulp of a below a tie")
    # the same with the sample carrying the scale: d = q 2^k as a float32
    k = rng.integers(-20, 21, n).astype(np.float64)
    check_fma(d * 2.0 ** k, t * 2.0 ** -k, a, "ties, scaled samples")


def test_fma_float32_extremes():
    rng = np.random.default_rng(504)
    n = 4000
    sub = rng.integers(1, 1 << 23, n).astype(np.uint32).view(np.float32).astype(np.float64) * rng.choice([-1.0, 1.0], n)
    big = rng.choice([3e38, -3e38, float(np.finfo(np.float32).max)], n).astype(np.float32).astype(np.float64)
    t = rng.uniform(-1.0, 1.0, n)
    for d, what in ((sub, "float32 subnormals"), (big, "3e38")):
        check_fma(d, t, np.zeros(n), what + ", a = 0")
        check_fma(d, t, -(d * t), what + ", cancelling")
        check_fma(d, t, d * t * rng.uniform(-2.0, 2.0, n), what + ", a of the product's size")
        check_fma(d, t, rng.uniform(-1.5, 1.5, n), what + ", a of an ordinary sample's size")
    check_fma(big, t, sub, "3e38 with a subnormal a")


def test_fma_zeros_of_both_signs():
    vals_d, vals_t, vals_a = (0.0, -0.0, 1.5, -1.5), (0.0, -0.0, 0.25, -0.25), (0.0, -0.0, 0.375, -0.375, 1.0)
    d, t, a = (np.array(v) for v in zip(*itertools.product(vals_d, vals_t, vals_a)))
    check_fma(d, t, a, "zeros")
    got = om.fma64(d, t, a)
    assert np.array_equal(np.signbit(got), np.signbit(d * t + a))         # every product here is exact
    assert np.signbit(om.fma64(-0.0, 0.25, -0.0)) and not np.signbit(om.fma64(-0.0, 0.25, 0.0)) and not np.signbit(om.fma64(1.5, 0.25, -0.375))


def test_fma_operands_that_are_not_finite_follow_ieee():
    inf, nan = np.inf, np.nan
    d = np.array([inf, -inf, nan, 1.0, 1.0, inf, 0.0, inf])
    t = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0])
    a = np.array([1.0, 1.0, 1.0, inf, nan, -inf, inf, 1.0])
    got = om.fma64(d, t, a)
    want = np.array([inf, -inf, nan, inf, nan, nan, inf, nan])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])


# ---------------------------------------------------------------------------------------------------------------------------
# the rows of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(fmrx):
    return fmrx.metersTable(mc.IF_FS)


@pytest.fixture(scope="module")
def fixtures(oracle):
    """test -> [(name, float32 row)]; rows of one test in the order the power check tries them"""
    f = {"a": [(f"M={M} tail={tail} row {c}", r) for M, tail in mc.A_CASES for c, r in enumerate(mc.a_rows(M, tail))],
         "c": [(f"n_if={n} row {c}", r) for n in mc.C_LENGTHS for c, r in enumerate(mc.c_rows(n))]}
    for nb in mc.B_BASE_CHOICES:      # the device's CU count decides which of the two the GPU test uses
        f[f"b{nb}"] = [(f"n_if={n} base row {c} of {nb}", r) for n in mc.B_LENGTHS for c, r in enumerate(mc.b_rows(nb, n))]
    d = []
    for c, iq in enumerate(mc.d_streams()):
        row = oracle.pipeline(0, 2).process(iq)["demod"]
        assert len(row) == 75 * L and np.isfinite(row).all()
        d += [(f"channel {c}", row), (f"channel {c}, {mc.D_SHORT} samples short", row[:-mc.D_SHORT])]
    f["d"] = d
    return f


TESTS = ("a",) + tuple(f"b{nb}" for nb in mc.B_BASE_CHOICES) + ("c", "d")
_model_cache = {}


def ordered(name, row, table, mutant=None):
    key = (name, len(row), mutant)
    if key not in _model_cache:
        _model_cache[key] = om.mpx_ordered(row, *table, mutant)
    return _model_cache[key]


@pytest.mark.parametrize("test", TESTS)
def test_order_model_meets_the_definition(fixtures, table, test):
    """finite rows: within the bounds tests/test_gpu_meters.py allows the device (a reordering of the same sums); rows that are
    not finite: the rule of the model's docstring"""
    worst = np.zeros(3)
    for name, row in fixtures[test]:
        got = ordered(test + name, row, table)
        assert np.all(got["probe"][5:] == 0.0), name
        x = row.astype(np.float64)
        if not np.isfinite(x).all():
            assert got["max_abs"] == np.nanmax(np.abs(x)), name
            assert not np.isfinite(got["sum_x"]) and not np.isfinite(got["sum_x2"]), name
            M, bad = len(x) // L, np.flatnonzero(~np.isfinite(x))
            assert (not np.isfinite(got["probe"][:5]).any()) if (bad < M * L).any() else np.isfinite(got["probe"]).all(), name
            continue
        want = mm.mpx_group(row, mc.IF_FS)
        assert got["max_abs"] == want["max_abs"], name
        e = (abs(got["sum_x"] - want["sum_x"]) / want["sum_abs"], abs(got["sum_x2"] - want["sum_x2"]) / want["sum_x2"],
             np.abs(got["probe"] - want["probe"]).max() / want["bound"])
        worst = np.maximum(worst, e)
        assert max(e) <= mm.REL, f"{name}: {e}"
    print(f"test {test}: largest sum_x, sum_x2, probe difference relative to its scale: {worst} (bound {mm.REL})")


def test_rows_that_are_not_finite_read_as_stated(table):
    """case (c)'s rows: NaN in a segment -> sums and probes NaN, max_abs the largest of the rest; +inf in a segment and -inf in
    the tail -> sum_x NaN (inf - inf), sum_x2 +inf, max_abs +inf, probes not finite; no sample that is not NaN -> 0"""
    x = mc.c_rows(mc.C_LENGTHS[0])
    r0, r1 = om.mpx_ordered(x[0], *table), om.mpx_ordered(x[1], *table)
    assert np.isnan(r0["sum_x"]) and np.isnan(r0["sum_x2"]) and np.isnan(r0["probe"][:5]).all()
    assert np.isfinite(r0["max_abs"]) and r0["max_abs"] == float(np.nanmax(np.abs(x[0])))
    assert np.isnan(r1["sum_x"]) and r1["sum_x2"] == np.inf and r1["max_abs"] == np.inf and not np.isfinite(r1["probe"][:5]).any()
    nothing = om.mpx_ordered(np.full(L + 3, np.nan, np.float32), *table)
    assert nothing["max_abs"] == 0.0 and not np.signbit(nothing["max_abs"])
    tail_only = x[3].copy()
    tail_only[-1] = np.nan                                      # in the tail: the probes do not see it
    r = om.mpx_ordered(tail_only, *table)
    assert np.isnan(r["sum_x"]) and np.array_equal(r["probe"], om.mpx_ordered(x[3], *table)["probe"])


# what a row needs for a mutant to have anything to change
APPLIES = {"unfused": lambda M, tail: True, "butterfly_rising": lambda M, tail: True, "waves_pairwise": lambda M, tail: True,
           "segments_reversed": lambda M, tail: M >= 3, "stale_buffer": lambda M, tail: M >= 33, "tail_first": lambda M, tail: tail > 0}


@pytest.mark.parametrize("mutant", om.MUTANTS)
@pytest.mark.parametrize("test", TESTS)
def test_each_mutant_changes_the_bits(fixtures, table, test, mutant):
    """on at least one row of each GPU test, in at least one compared field"""
    assert set(APPLIES) == set(om.MUTANTS)
    tried = 0
    for name, row in fixtures[test]:
        if not APPLIES[mutant](len(row) // L, len(row) % L):
            continue
        tried += 1
        fields = mc.differing_fields(ordered(test + name, row, table, mutant), ordered(test + name, row, table))
        if fields:
            print(f"test {test}, {mutant}: {name}: {', '.join(fields)} differ (row {tried} tried)")
            return
    pytest.fail(f"test {test}: the mutant {mutant} changes no bit on any of its {tried} applicable rows")
