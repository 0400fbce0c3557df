"""The rational-rate tuner's integer model (tests/_tuner_rational_model.py) against its float64 statement, against the integer
models it extends (U = 1), against the product's host code (fmrx_tuner_design_rational), and what the rates are for: the
default prototype's figures, the selectivity of a 10 MS/s int16 capture through 6/25, and the CPU statement of that capture's
way through tuner, bank and RDS chain, against which tests/test_gpu_tuner_rational_bank.py measures the device.  No GPU."""
import os
import sys
from math import gcd

import numpy as np
import pytest

import _rds_station_model as SM
import _tuner_formats_model as fm
import _tuner_model as tm
import _tuner_rational_capture as RC
import _tuner_rational_model as rm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rds_oracle  # noqa: E402

FORMATS = [fm.U8, fm.S8, fm.S16]
ids = lambda f: fm.NAMES[f] if isinstance(f, int) and f in fm.NAMES else None   # noqa: E731
RATIOS = [(2, 5), (3, 10), (6, 25), (3, 25), (18, 125)]


def capture_rate(U, D):
    """the capture rate a ratio is for: 10 MS/s -> 1.44 MS/s for 18/125, otherwise whatever gives 2.4 MS/s"""
    return 10e6 if (U, D) == (18, 125) else 2.4e6 * D / U


def low_pass(oracle, Fs_w, U, D, T):
    """tunerLowPassRational's rule through the oracle's filter design"""
    rf_Fs = Fs_w * U / D
    return (np.float32(U) * oracle.impulse_response_lpf(U * Fs_w, 0.5 * (128e3 + rf_Fs - 100e3), T)).astype(np.float32)


def random_raw(rng, n_values, fmt):
    lo, hi = fm.FULL_SCALE[fmt]
    return rng.integers(lo, hi + 1, n_values).astype(fm.DTYPES[fmt])


# (f_c / Fs_w, amplitude, tone): 0.3 Fs_w apart, beyond the prototype's transition band even at 2/5, where Fs_w is 2.5 rf_Fs
STATIONS = [(-0.3, 0.5, 1000.0), (0.0, 0.1, 2500.0), (0.3, 0.02, 4000.0)]


def three_stations(fmt, Fs_w, n_wide):
    """faded in over the first eighth: a capture that starts at full level is a step, and the step of the strong station
    overshoots through the weak one's filter (it clips there at a gain of 35); a receiver's capture does not start like that"""
    z = sum(fm.fm_station(n_wide, Fs_w, f * Fs_w, a, t) for f, a, t in STATIONS)
    ramp = np.minimum(1.0, np.arange(n_wide) / (n_wide / 8.0))
    return fm.quantise(z * (0.5 - 0.5 * np.cos(np.pi * ramp)), fmt)


# ---- the float64 statement ------------------------------------------------------------------------------------------------
def check_against_f64(values, fmt, h, U, D, Fs_w, f_c, gain, n0=0):
    """model bytes vs clip(128 + tuner_rational_f64), sample by sample -> (largest error, smallest margin, clipped)"""
    Tp = -(-len(h) // U)
    hist = fm.silence(Tp, fmt)
    w, s, re, im = rm.design(h, U, Fs_w, f_c, gain)
    cps = f_c / Fs_w
    ar, ai = rm.accumulate(values, hist, re, im, U, D, fmt)
    out, clipped, power = rm.rotate_round(ar[0], ai[0], w, s, U, D, n0, fmt)
    y = rm.tuner_rational_f64(values, hist, h, U, D, cps, gain, fmt, n0)
    b = np.repeat(rm.tuner_rational_bound(values, hist, re, im, w, s, U, D, cps, fmt, n0), 2)
    want = np.empty(2 * len(y))
    want[0::2], want[1::2] = 128.0 + y.real, 128.0 + y.imag
    d = np.abs(out.astype(np.float64) - np.clip(want, 0.0, 255.0))
    worst = int(np.argmax(d - b))
    assert np.all(d <= b), f"byte {worst}: model {out[worst]} vs float64 {want[worst]:.6f}, bound {b[worst]:.4f}"
    d2 = out.astype(np.int64) - 128
    assert power == int((d2 * d2).sum())
    return float(d.max()), float((b - d).min()), clipped


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("U,D", RATIOS)
def test_model_within_the_derived_bound_of_float64(oracle, U, D, fmt):
    Fs_w, T = capture_rate(U, D), 8 * D
    h = low_pass(oracle, Fs_w, U, D, T)
    rng = np.random.default_rng(1000 * U + 10 * D + fmt)
    lo, hi = fm.FULL_SCALE[fmt]
    dt = fm.DTYPES[fmt]
    n = D * 40
    # the three stations, each tuned with the gain that brings it to 90 of 127 LSB: the model itself must clip nothing there
    smallest = np.inf
    cap = three_stations(fmt, Fs_w, n)
    for f, a, _ in STATIONS:
        err, margin, clipped = check_against_f64(cap, fmt, h, U, D, Fs_w, f * Fs_w, 90.0 / 127.0 / a)
        assert clipped == 0, f"three stations, f_c = {f} Fs_w: the model clips {clipped} bytes"
        smallest = min(smallest, margin)
        print(f"{fm.NAMES[fmt]} {U}/{D} three stations f_c={f:+.2f} Fs_w: max error {err:.4f} LSB, margin {margin:.4f}")
    for name, values in {"random": random_raw(rng, 2 * n, fmt), "all minimum": np.full(2 * n, lo, dt), "all maximum": np.full(2 * n, hi, dt)}.items():
        for f_c, gain in [(0.0, 0.9), (0.13 * Fs_w, 0.9), (-0.16 * Fs_w, 1.8), (-0.44 * Fs_w, 3.0), (0.4958 * Fs_w, 40.0)]:
            err, margin, clipped = check_against_f64(values, fmt, h, U, D, Fs_w, f_c, gain)
            smallest = min(smallest, margin)
            print(f"{fm.NAMES[fmt]} {U}/{D} {name} f_c={f_c:+.0f} gain={gain}: max error {err:.4f} LSB, margin {margin:.4f}, clipped {clipped}")
    print(f"{fm.NAMES[fmt]} {U}/{D}: smallest margin {smallest:.4f} LSB")
    assert smallest > 0.0


def test_float64_statement_equals_the_polyphase_form():
    """the identity the definition rests on: zero-stuff, filter, keep every D-th == the per-phase sum (*), in float64"""
    rng = np.random.default_rng(11)
    for U, D, T in [(2, 5, 13), (3, 10, 80), (6, 25, 200), (7, 15, 3)]:
        Tp = -(-T // U)
        h = rng.standard_normal(T).astype(np.float32)
        values = random_raw(rng, 2 * D * 30, fm.S8)
        hist = random_raw(rng, 2 * (Tp - 1), fm.S8)
        y = rm.tuner_rational_f64(values, hist, h, U, D, 0.0, 1.0, fm.S8)
        x = np.concatenate([fm.to_x(hist, fm.S8), fm.to_x(values, fm.S8)]).astype(np.float64)
        z = x[0::2] + 1j * x[1::2]
        hp = rm.phase_taps(h, U)
        nm, pm = rm.out_times(len(y), U, D)
        want = np.array([sum(hp[p, j] * z[Tp - 1 + n - j] for j in range(Tp)) for n, p in zip(nm, pm)])
        assert np.abs(y - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


# ---- U = 1 is the integer tuner ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("R", [4, 8, 10])
def test_u_1_is_the_integer_model_byte_for_byte(oracle, R, fmt):
    Fs_w, T, N = 2.4e6 * R, 8 * R + 1, 3
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T)
    a, b = rm.TunerRationalModel(h, 1, R, N, fmt), fm.TunerModel(h, R, N, fmt)
    u8 = tm.TunerModel(h, R, N) if fmt == fm.U8 else None
    for c, (f_c, g) in enumerate([(0.0, 1.0), (0.31 * Fs_w, 2.0), (-0.46 * Fs_w, 45.0)]):
        for m in (a, b, u8):
            if m is not None:
                m.set_channel(c, f_c, Fs_w, g)
        assert (a.w[c], a.s[c]) == (b.w[c], b.s[c]) and np.array_equal(a.re[c], b.re[c]) and np.array_equal(a.im[c], b.im[c])
    rng = np.random.default_rng(R + fmt)
    for n_out in (1, 7, 300):
        values = random_raw(rng, 2 * R * n_out, fmt)
        got, want = a.process(values), b.process(values)
        assert np.array_equal(got, want)
        assert np.array_equal(a.clipped, b.clipped) and np.array_equal(a.power, b.power)
        if u8 is not None:
            assert np.array_equal(got, u8.process(values)) and np.array_equal(a.clipped, u8.clipped) and np.array_equal(a.power, u8.power)
    assert b.clipped[2] > 0
    assert a.n == b.n and np.array_equal(a.hist, b.hist)


# ---- cuts and formats ---------------------------------------------------------------------------------------------------
def plan3(model, Fs_w):
    for c, (f_c, g) in enumerate([(0.0, 1.0), (0.31 * Fs_w, 2.0), (-0.46 * Fs_w, 0.7)]):
        model.set_channel(c, f_c, Fs_w, g)


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("U,D,T", [(2, 5, 9), (6, 25, 200), (18, 125, 77)])
def test_cut_invariance(oracle, U, D, T, fmt):
    Fs_w = capture_rate(U, D)
    h = low_pass(oracle, Fs_w, U, D, T)
    values = random_raw(np.random.default_rng(5), 2 * D * 70, fmt)
    whole_m = rm.TunerRationalModel(h, U, D, 3, fmt)
    plan3(whole_m, Fs_w)
    whole = whole_m.process(values)
    assert whole.shape == (3, 2 * 70 * U)
    m = rm.TunerRationalModel(h, U, D, 3, fmt)
    plan3(m, Fs_w)
    parts, pos = [], 0
    for periods in (1, 2, 7, 1, 30, 29):
        parts.append(m.process(values[pos:pos + 2 * D * periods]))
        pos += 2 * D * periods
    assert pos == len(values)
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert m.n == whole_m.n and np.array_equal(m.hist, whole_m.hist)


@pytest.mark.parametrize("U,D,T", [(2, 5, 9), (3, 10, 80), (6, 25, 200), (18, 125, 1000)])
def test_the_two_format_identities(oracle, U, D, T):
    """S8 fed b equals U8 fed b ^ 0x80; S16 fed (u8 - 128) << 8 equals U8 fed the u8 -- bytes and levels"""
    Fs_w = capture_rate(U, D)
    h = low_pass(oracle, Fs_w, U, D, T)
    models = {f: rm.TunerRationalModel(h, U, D, 3, f) for f in FORMATS}
    for m in models.values():
        plan3(m, Fs_w)
        m.set_channel(2, -0.46 * Fs_w, Fs_w, 45.0)
    rng = np.random.default_rng(U * D)
    for periods in (1, 9, 50):
        u8 = rng.integers(0, 256, 2 * D * periods, dtype=np.uint8)
        want = models[fm.U8].process(u8)
        assert np.array_equal(models[fm.S8].process((u8 ^ 0x80).view(np.int8)), want)
        assert np.array_equal(models[fm.S16].process(((u8.astype(np.int32) - 128) << 8).astype(fm.DTYPES[fm.S16])), want)
        for f in (fm.S8, fm.S16):
            assert np.array_equal(models[f].clipped, models[fm.U8].clipped) and np.array_equal(models[f].power, models[fm.U8].power)
    assert models[fm.U8].clipped[2] > 0


# ---- the product's host code -------------------------------------------------------------------------------------------
def same_or_tie(got, v):
    """got int16 equals llround(v), except by one unit where v is within 1e-9 of a half-integer (a libm tie)"""
    want = tm.llround(v)
    diff = got.astype(np.int64) - want
    frac = np.abs(v) - np.floor(np.abs(v))
    return bool(((diff == 0) | ((np.abs(diff) == 1) & (np.abs(frac - 0.5) < 1e-9))).all())


def test_design_rational_equals_the_model(fmrx, oracle):
    rng = np.random.default_rng(7)
    n = 0
    # T = 8 D; T no multiple of U (ragged last taps); T < U (Tp = 1, some phases all zero); U = 1
    for U, D, T in [(2, 5, 40), (3, 10, 80), (6, 25, 200), (18, 125, 1000), (6, 25, 199), (18, 125, 77), (3, 10, 2), (18, 125, 5), (32, 67, 31),
                    (1, 8, 64)]:
        Fs_w = capture_rate(U, D)
        h = low_pass(oracle, Fs_w, U, D, T) if T > 5 else np.array([0.5, 0.25, -0.125, 1.0, 0.75][:T], np.float32)
        Tp = -(-T // U)
        cases = [(0.0, 1.0), (100e3, 1.0), (-100e3, 2.5), (Fs_w / 2 - 1.0, 1.0), (-Fs_w / 2 + 1.0, 0.3), (123456.789, 1e-3), (-7.0, 1e4)]
        cases += [(float(rng.uniform(-0.499, 0.499) * Fs_w), float(10 ** rng.uniform(-3, 3))) for _ in range(6)]
        for f_c, gain in cases:
            w, s, re, im = fmrx.Tuner.design_rational(h, U, Fs_w, f_c, gain)
            mw, ms, vr, vi = rm.design_f64(h, U, Fs_w, f_c, gain)
            assert len(re) == len(im) == U * Tp
            assert w == mw and w == tm.freq_word(f_c, Fs_w), f"frequency word, f_c={f_c}"
            assert s == ms, f"scale exponent, {U}/{D} T={T} f_c={f_c} gain={gain}"
            assert same_or_tie(re, vr.reshape(-1)) and same_or_tie(im, vi.reshape(-1)), f"taps, {U}/{D} T={T} f_c={f_c} gain={gain}"
            assert max(np.abs(re).max(), np.abs(im).max()) <= tm.LIMIT
            if T < U:
                assert not re.reshape(U, Tp)[T:].any() and not im.reshape(U, Tp)[T:].any(), "phases past the prototype are zero"
            n += 1
        if U == 1:                                                 # and the integer design, integer for integer
            w1, s1, re1, im1 = fmrx.Tuner.design(h, Fs_w, 123456.789, 0.7)
            w2, s2, re2, im2 = fmrx.Tuner.design_rational(h, 1, Fs_w, 123456.789, 0.7)
            assert (w1, s1) == (w2, s2) and np.array_equal(re1, re2) and np.array_equal(im1, im2)
    assert n == 10 * 13


def test_design_rational_rejects_what_the_model_rejects(fmrx):
    h = np.hanning(34)[1:-1].astype(np.float32)
    hn = h.copy()
    hn[3] = np.nan
    bad = [(np.zeros(32, np.float32), 3, 1e6, 0.0, 1.0), (h, 3, 1e6, 0.0, 0.0), (h, 3, 1e6, 0.5e6, 1.0), (h, 3, 1e6, -0.5e6, 1.0),
           (h, 3, 1e6, 0.0, float("nan")), (h, 3, 1e6, 0.0, float("inf")), (h, 3, 1e6, 0.0, 1e-30), (h, 3, 1e6, 0.0, 1e30),
           (hn, 3, 1e6, 0.0, 1.0), (h, 0, 1e6, 0.0, 1.0), (h, 33, 1e6, 0.0, 1.0),
           (np.ones(3000, np.float32), 3, 1e6, 0.123e6, 1.0)]     # 1000 taps per phase: a phase's accumulator overflows
    for hh, U, Fs_w, f_c, gain in bad:
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.Tuner.design_rational(hh, U, Fs_w, f_c, gain)
        assert e.value.code == fmrx.EINVAL
        with pytest.raises(ValueError):
            rm.design(hh, U, Fs_w, f_c, gain)
    # the worst case is per PHASE: the 3000 ones a phase of which overflows pass when they spread over 12 phases, although
    # the sum over all taps is the same
    w, s, re, im = fmrx.Tuner.design_rational(np.ones(3000, np.float32), 12, 1e6, 0.123e6, 1.0)
    per_phase = (np.abs(re.astype(np.int64)) + np.abs(im.astype(np.int64))).reshape(12, 250).sum(axis=1)
    assert 128 * int(per_phase.max()) < 2 ** 31 <= 128 * int(per_phase.sum())
    mw, ms, mre, mim = rm.design(np.ones(3000, np.float32), 12, 1e6, 0.123e6, 1.0)
    assert (w, s) == (mw, ms)


def test_ratio_and_scale_exponent_ranges(oracle):
    """gcd != 1, U and D out of range, D < 2 U; s within -14 .. 47, -14 .. 39 for S16"""
    h = low_pass(oracle, 10e6, 6, 25, 200)
    for U, D in [(6, 24), (2, 4), (0, 5), (33, 67), (6, 11), (1, 1), (3, 513), (5, 25)]:
        with pytest.raises(ValueError):
            rm.TunerRationalModel(h, U, D, 1)
    for U, D in [(1, 2), (32, 65), (6, 25), (1, 512), (24, 125)]:
        assert gcd(U, D) == 1
        rm.check_ratio(U, D)
    by_s = {}
    for e in np.arange(-11.0, 10.0, 0.05):
        w, s, vr, vi = rm.design_f64(h, 6, 10e6, 1e6, 10.0 ** e)
        if s is not None:
            by_s.setdefault(s, 10.0 ** e)
    assert {-14, 39, 40, 47} <= set(by_s) and min(by_s) == -14 and max(by_s) == 47
    m16, m8 = rm.TunerRationalModel(h, 6, 25, 1, fm.S16), rm.TunerRationalModel(h, 6, 25, 1, fm.S8)
    values = random_raw(np.random.default_rng(8), 2 * 25 * 30, fm.S16)
    for s in (-14, 39):
        m16.set_channel(0, 1e6, 10e6, by_s[s])
        assert m16.s[0] == s
        m16.process(values)
    for s in (40, 47):
        with pytest.raises(ValueError):
            m16.set_channel(0, 1e6, 10e6, by_s[s])
        m8.set_channel(0, 1e6, 10e6, by_s[s])
    assert m16.s[0] == 39


# ---- the default prototype ----------------------------------------------------------------------------------------------
# (U, D, Fs_w, |response at 128 kHz against DC| dB, stop band dB): the figures of tunerLowPassRational's docstring, which are
# rounded to 0.001 dB and 0.1 dB; the test allows that rounding, half a unit of the last digit
LOW_PASS_FIGURES = [(6, 25, 10e6, 0.011, -62.4), (3, 25, 20e6, 0.011, -62.4), (24, 125, 12.5e6, 0.011, -62.4), (3, 10, 8e6, 0.011, -62.4),
                    (3, 20, 16e6, 0.011, -62.4), (18, 125, 10e6, 0.023, -61.2), (12, 125, 10e6, 0.032, -54.9)]


@pytest.mark.parametrize("U,D,Fs_w,pass_db,stop_db", LOW_PASS_FIGURES)
def test_tuner_low_pass_rational_meets_its_figures(fmrx, U, D, Fs_w, pass_db, stop_db):
    T = 8 * D
    h = fmrx.tunerLowPassRational(Fs_w, U, D, T)
    assert h.dtype == np.float32 and len(h) == T
    rf_Fs = Fs_w * U / D
    assert np.array_equal(h, (np.float32(U) * fmrx.impulseResponseLPF(U * Fs_w, 0.5 * (128e3 + rf_Fs - 100e3), T)).astype(np.float32))
    hd = h.astype(np.float64)
    k = np.arange(T)
    resp = lambda f: np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), k) / (U * Fs_w)) @ hd)   # noqa: E731
    dc = resp(0.0)[0]
    assert abs(dc / U - 1.0) < 2e-3, "unity pass band after zero-stuffing by U"
    at128 = 20 * np.log10(resp(128e3)[0] / dc)
    stop = 20 * np.log10(resp(np.linspace(rf_Fs - 100e3, U * Fs_w / 2, 4000)).max() / dc)
    print(f"{U}/{D} at {Fs_w / 1e6} MS/s, T = {T}: {at128:+.4f} dB at 128 kHz, stop band {stop:.1f} dB")
    assert abs(at128) <= pass_db + 0.0005 and stop <= stop_db + 0.05


# ---- selectivity: a 10 MS/s int16 capture through 6/25 against the integer tuner at 9.6 MS/s, R = 4 ------------------------
def test_selectivity_of_a_10_ms_capture_through_6_25(fmrx):
    """A full-deviation station at 0.5 of full scale and one 60 dB below it carrying a 1 kHz tone, 20 ms as int16: tuned to the
    weak one by the rational model (10 MS/s, 6/25, T = 200) and, the same signal sampled at 9.6 MS/s, by the integer model
    (R = 4, T = 32); the tone-to-residual ratio of the rational path has to be within 3 dB of the integer one (the margin
    covers the prototypes' different transition bands).  The stations sit at +1.2 and -2.0 MHz: 3.2 MHz apart and inside
    +-4.8 MHz, so that neither rate folds one of them and both tuners see the strong station at the same offset."""
    f_s, a_s, t_s, f_w, tone = 1.2e6, 0.5, 2500.0, -2.0e6, 1000.0
    a_w = a_s * 10.0 ** (-60 / 20)
    fig = {}
    for name, Fs_w, n_wide in [("rational 6/25 at 10 MS/s", 10e6, 200_000), ("integer R = 4 at 9.6 MS/s", 9.6e6, 192_000)]:
        z = fm.fm_station(n_wide, Fs_w, f_s, a_s, t_s) + fm.fm_station(n_wide, Fs_w, f_w, a_w, tone)
        values = fm.quantise(z, fm.S16)
        if Fs_w == 10e6:
            m = rm.TunerRationalModel(fmrx.tunerLowPassRational(Fs_w, 6, 25, 200), 6, 25, 1, fm.S16)
        else:
            m = fm.TunerModel(fmrx.tunerLowPass(Fs_w, 4, 32), 4, 1, fm.S16)
        m.set_channel(0, f_w, Fs_w, 0.7 / a_w)
        out = m.process(values)[0]
        assert len(out) == 2 * 48000
        fig[name] = fm.tone_fit_db(out, 2.4e6, tone)
        print(f"weak / strong -60 dB, {name}: tone fit {fig[name]:.1f} dB, {int(m.clipped[0])} of {len(out)} output bytes clamp")
    r, i = fig["rational 6/25 at 10 MS/s"], fig["integer R = 4 at 9.6 MS/s"]
    assert abs(r - i) <= 3.0, f"rational {r:.1f} dB, integer {i:.1f} dB"


# ---- the CPU statement of 10 MS/s int16 capture -> 6/25 -> bank -> RDS ---------------------------------------------------
def test_rds_capture_at_10_ms_decodes_on_the_cpu(fmrx, oracle):
    """rational model (S16, 6/25, tunerLowPassRational at T = 200) -> the oracle's mode-0 discriminator ->
    rds_oracle.RdsChain -> the station model, for the three stations of one capture; no tuned byte clipped"""
    c = RC.RDS
    s16 = RC.rds_capture_10ms_s16()
    assert np.abs(s16.astype(np.int32)).max() < 32767
    h = fmrx.tunerLowPassRational(c["Fs_w"], c["U"], c["D"], c["T"])
    m = rm.TunerRationalModel(h, c["U"], c["D"], 3, fm.S16)
    for k in range(3):
        m.set_channel(k, c["offsets"][k], c["Fs_w"], RC.rds_gain(k))
    chains = [(oracle.pipeline(0, 1), rds_oracle.RdsChain(upsamp=247, decim=960, sps=26), SM.StationModel(26)) for _ in range(3)]
    step = 2 * RC.N_WIDE_PER_CALL
    right, clipped = [], 0
    for i in range(c["calls"]):
        out = m.process(s16[i * step:(i + 1) * step])
        assert out.shape == (3, c["bytes_per_call"])
        clipped += int(m.clipped.sum())
        row = []
        for k, (pl, chain, st) in enumerate(chains):
            st.feed_rrc(chain.process(pl.process(out[k])["demod"])["rrc_i"])
            row.append(st.pi == c["pi"][k] and bytes(st.ps).decode("latin-1") == c["ps"][k])
        right.append(row)
    since = [next((i + 1 for i in range(len(right)) if all(r[k] for r in right[i:])), None) for k in range(3)]
    print(f"PI and PS right from calls {since}; tuned bytes clipped: {clipped}")
    assert clipped == 0
    assert all(s is not None and s <= RC.RIGHT_FROM_CALL for s in since), f"PI / PS right from calls {since}"
