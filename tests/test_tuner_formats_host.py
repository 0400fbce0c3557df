"""The wideband tuner's input formats on the CPU: the integer model of signed 8-bit and 16-bit captures
(tests/_tuner_formats_model.py) against the two identities that tie it to the u8 model, against the float64 statement of
the same mathematics, and on what the 16-bit format is for -- a weak station beside a strong one.  No GPU involved."""
import numpy as np
import pytest

import _tuner_capture as TC
import _tuner_formats_model as fm
import _tuner_model as tm

FORMATS = [fm.S8, fm.S16]
ids = [fm.NAMES[f] for f in FORMATS]


def random_raw(rng, n_values, fmt):
    lo, hi = fm.FULL_SCALE[fmt]
    return rng.integers(lo, hi + 1, n_values).astype(fm.DTYPES[fmt])


def plan3(model, Fs_w, R):
    for c, (f_c, g) in enumerate([(0.0, 1.0), (0.9e6 * R, 2.0), (-1.1e6 * R, 45.0)]):
        model.set_channel(c, f_c, Fs_w, g)


# ---- the identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T", [(4, 33), (8, 64), (10, 80), (20, 2)])
def test_s8_equals_u8_on_the_flipped_bytes(oracle, R, T):
    Fs_w = 2.4e6 * R
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T) if T > 2 else np.array([0.5, 0.5], np.float32)
    rng = np.random.default_rng(R)
    a, b = tm.TunerModel(h, R, 3), fm.TunerModel(h, R, 3, fm.S8)
    plan3(a, Fs_w, R)
    plan3(b, Fs_w, R)
    for n_out in (1, 50, 333):
        u8 = rng.integers(0, 256, 2 * R * n_out, dtype=np.uint8)
        assert np.array_equal(a.process(u8), b.process((u8 ^ 0x80).view(np.int8)))
        assert np.array_equal(a.clipped, b.clipped) and np.array_equal(a.power, b.power)
    assert a.clipped[2] > 0


@pytest.mark.parametrize("R,T", [(4, 33), (8, 64), (10, 80), (20, 2)])
def test_s16_equals_u8_on_the_bytes_shifted_up(oracle, R, T):
    Fs_w = 2.4e6 * R
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T) if T > 2 else np.array([0.5, 0.5], np.float32)
    rng = np.random.default_rng(100 + R)
    a, b = tm.TunerModel(h, R, 3), fm.TunerModel(h, R, 3, fm.S16)
    plan3(a, Fs_w, R)
    plan3(b, Fs_w, R)
    for n_out in (1, 50, 333):
        u8 = rng.integers(0, 256, 2 * R * n_out, dtype=np.uint8)
        s16 = ((u8.astype(np.int32) - 128) << 8).astype(fm.DTYPES[fm.S16])
        assert np.array_equal(a.process(u8), b.process(s16))
        assert np.array_equal(a.clipped, b.clipped) and np.array_equal(a.power, b.power)
    assert a.clipped[2] > 0


def test_u8_through_the_formats_model_is_the_u8_model(oracle):
    R, T, Fs_w = 8, 64, 19.2e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    a, b = tm.TunerModel(h, R, 3), fm.TunerModel(h, R, 3, fm.U8)
    plan3(a, Fs_w, R)
    plan3(b, Fs_w, R)
    u8 = np.random.default_rng(1).integers(0, 256, 2 * R * 500, dtype=np.uint8)
    assert np.array_equal(a.process(u8), b.process(u8)) and np.array_equal(a.power, b.power)


def test_a_wrong_dtype_is_refused(oracle):
    m = fm.TunerModel(np.array([0.5, 0.5], np.float32), 4, 1, fm.S16)
    with pytest.raises(AssertionError):
        m.process(np.zeros(16, np.uint8))


# ---- the float64 statement ------------------------------------------------------------------------------------------------
def check_against_f64(values, fmt, h, R, Fs_w, f_c, gain, n0=0):
    """model bytes vs clip(128 + tuner_f64), sample by sample -> (largest error, smallest margin, clipped, largest |acc|)"""
    T = len(h)
    hist = fm.silence(T, fmt)
    w, s, re, im = tm.design(h, Fs_w, f_c, gain)
    cps = f_c / Fs_w
    ar, ai = fm.accumulate(values, hist, re, im, R, fmt)
    out, clipped, power = fm.rotate_round(ar[0], ai[0], w, s, R, n0, fmt)
    y = fm.tuner_f64(values, hist, h, R, cps, gain, fmt, n0)
    b = np.repeat(fm.tuner_bound(values, hist, re, im, w, s, R, cps, fmt, n0), 2)
    want = np.empty(2 * len(y))
    want[0::2], want[1::2] = 128.0 + y.real, 128.0 + y.imag
    d = np.abs(out.astype(np.float64) - np.clip(want, 0.0, 255.0))
    worst = int(np.argmax(d - b))
    assert np.all(d <= b), f"byte {worst}: model {out[worst]} vs float64 {want[worst]:.6f}, bound {b[worst]:.4f}"
    d2 = out.astype(np.int64) - 128
    assert power == int((d2 * d2).sum())
    return float(d.max()), float((b - d).min()), clipped, int(max(np.abs(ar).max(), np.abs(ai).max()))


def multi_station(fmt, R, n_wide):
    """three FM stations of unequal level in one capture of the format"""
    Fs_w = 2.4e6 * R
    z = sum(fm.fm_station(n_wide, Fs_w, f * Fs_w, a, t) for f, a, t in [(-0.16, 0.5, 1000.0), (0.02, 0.1, 2500.0), (0.27, 0.02, 4000.0)])
    return fm.quantise(z, fmt)


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("R", [4, 8, 10, 20])
def test_model_within_the_derived_bound_of_float64(oracle, R, fmt):
    Fs_w, T = 2.4e6 * R, 8 * R + 1
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T)
    rng = np.random.default_rng(10 * R + fmt)
    lo, hi = fm.FULL_SCALE[fmt]
    dt = fm.DTYPES[fmt]
    inputs = {"random": random_raw(rng, 2 * R * 3000, fmt), "all minimum": np.full(2 * R * 500, lo, dt),
              "all maximum": np.full(2 * R * 500, hi, dt), "multi-station": multi_station(fmt, R, R * 3000)}
    top = 0
    for name, values in inputs.items():
        for f_c, gain in [(0.0, 0.9), (0.31e6 * R, 0.9), (-0.16 * Fs_w, 1.8), (-1.05e6 * R, 3.0), (-1.19e6 * R, 40.0)]:
            err, margin, clipped, big = check_against_f64(values, fmt, h, R, Fs_w, f_c, gain)
            top = max(top, big)
            print(f"{fm.NAMES[fmt]} R={R} {name} f_c={f_c:+.0f} gain={gain}: max error {err:.4f} LSB, margin {margin:.4f}, clipped {clipped}, |acc| <= 2^{np.log2(max(big, 1)):.1f}")
    if fmt == fm.S16:
        assert top >= 2 ** 31, "the S16 captures were meant to show that int32 does not hold acc"


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_bound_at_the_end_of_the_counter(oracle, fmt):
    R, T, Fs_w = 8, 64, 19.2e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    values = random_raw(np.random.default_rng(3), 2 * R * 400, fmt)
    w = tm.freq_word(5.2e6, Fs_w)
    # the frequency the word really stands for, so that the drift term does not swamp the check at n = 2^32
    f_exact = (w - 2 ** 32 if w >= 2 ** 31 else w) / 2.0 ** 32 * Fs_w
    assert tm.freq_word(f_exact, Fs_w) == w
    check_against_f64(values, fmt, h, R, Fs_w, f_exact, 1.5, n0=2 ** 32 - R * 400 - 8)


# ---- independence of call cuts, design, the range of s ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_cut_invariance(oracle, fmt):
    R, T, Fs_w = 10, 33, 24e6
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T)
    values = random_raw(np.random.default_rng(5), 2 * R * 700, fmt)
    whole_m = fm.TunerModel(h, R, 3, fmt)
    plan3(whole_m, Fs_w, R)
    whole = whole_m.process(values)
    m = fm.TunerModel(h, R, 3, fmt)
    plan3(m, Fs_w, R)
    parts, pos = [], 0
    for n_out in (1, 2, 7, 64, 300, 326):
        parts.append(m.process(values[pos:pos + 2 * R * n_out]))
        pos += 2 * R * n_out
    assert pos == len(values)
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert m.n == whole_m.n and np.array_equal(m.hist, whole_m.hist)


def test_design_does_not_depend_on_the_format(fmrx, oracle):
    """fmrx_tuner_design is unchanged: the integers of _tuner_model.py, and still every s of -14 .. 47 (an S16 tuner
    narrows the range when the channel is set, the design function has no format)"""
    R, T, Fs_w = 8, 64, 19.2e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    for f_c, gain in [(0.0, 1.0), (5.2e6, 0.7), (-3.1e6, 1400.0), (123456.789, 1e-3), (1e6, 1e-8), (1e6, 2e8)]:
        w, s, re, im = fmrx.Tuner.design(h, Fs_w, f_c, gain)
        mw, ms, mre, mim = tm.design(h, Fs_w, f_c, gain)
        assert (w, s) == (mw, ms)
        assert np.abs(re.astype(np.int64) - mre).max() <= 1 and np.abs(im.astype(np.int64) - mim).max() <= 1
    assert fmrx.Tuner.design(h, Fs_w, 1e6, 1e-8)[1] > fm.s_max(fm.S16)
    assert fmrx.TUNER_FORMATS == {"u8": fm.U8, "s8": fm.S8, "s16": fm.S16}


def test_s16_range_of_the_scale_exponent(oracle):
    """the shift s + 15 + 8 stays in 1 .. 62: -14 <= s <= 39 for S16, -14 <= s <= 47 for the 8-bit formats"""
    assert fm.s_max(fm.U8) == fm.s_max(fm.S8) == 47 and fm.s_max(fm.S16) == 39
    R, T, Fs_w = 8, 64, 19.2e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    by_s = {}
    for e in np.arange(-9.0, 10.0, 0.05):
        w, s, vr, vi = tm.design_f64(h, Fs_w, 1e6, 10.0 ** e)
        if s is not None:
            by_s.setdefault(s, 10.0 ** e)
    assert {-14, 39, 40, 47} <= set(by_s)
    m16, m8 = fm.TunerModel(h, R, 1, fm.S16), fm.TunerModel(h, R, 1, fm.S8)
    values = random_raw(np.random.default_rng(8), 2 * R * 300, fm.S16)
    for s in (-14, 39):
        m16.set_channel(0, 1e6, Fs_w, by_s[s])
        assert m16.s[0] == s
        m16.process(values)
    assert by_s[40] < 1e-7 / float(np.abs(h).max()), "a gain x tap product the S16 range excludes is below 1e-7"
    for s in (40, 47):
        with pytest.raises(ValueError):
            m16.set_channel(0, 1e6, Fs_w, by_s[s])
        m8.set_channel(0, 1e6, Fs_w, by_s[s])
    assert m16.s[0] == 39                                   # a refused channel keeps its settings


# ---- what the 16-bit format is for ---------------------------------------------------------------------------------------
NEAR_FAR = dict(Fs_w=19.2e6, R=8, T=64, strong=(5.2e6, 0.5, 2500.0), weak_f_c=-3.1e6, tone=1000.0, n_wide=8 * 48000)


def tuned(fmrx, values, fmt, f_c, gain):
    c = NEAR_FAR
    m = fm.TunerModel(fmrx.tunerLowPass(c["Fs_w"], c["R"], c["T"]), c["R"], 1, fmt)
    m.set_channel(0, f_c, c["Fs_w"], gain)
    return m.process(values)[0], int(m.clipped[0])


def test_near_far_a_weak_station_60_db_below_a_strong_one(fmrx):
    """One float capture, quantised once to int16 and once to u8: a full-deviation station at 0.5 of full scale at +5.2 MHz,
    and one 60 dB below it at -3.1 MHz carrying a 1 kHz tone, tuned with gain 0.7 / amplitude (R = 8, T = 64, tunerLowPass).
    Required: the tone fit of the int16 path >= 40 dB, of the u8 path <= 10 dB."""
    c = NEAR_FAR
    f_s, a_s, t_s = c["strong"]
    a_w = a_s * 10.0 ** (-60 / 20)
    z = fm.fm_station(c["n_wide"], c["Fs_w"], f_s, a_s, t_s) + fm.fm_station(c["n_wide"], c["Fs_w"], c["weak_f_c"], a_w, c["tone"])
    fig = {}
    for fmt in (fm.S16, fm.U8):
        out, clipped = tuned(fmrx, fm.quantise(z, fmt), fmt, c["weak_f_c"], 0.7 / a_w)
        fig[fmt] = fm.tone_fit_db(out, c["Fs_w"] / c["R"], c["tone"])
        print(f"weak / strong -60 dB, from the {fm.NAMES[fmt]} capture: tone fit {fig[fmt]:.1f} dB, {clipped} of {len(out)} output bytes clamp")
    assert fig[fm.S16] >= 40.0
    assert fig[fm.U8] <= 10.0


def test_a_lone_station_of_60_int16_units(fmrx):
    """below half a u8 LSB: every byte of the u8 capture is 128, the int16 path still gives >= 40 dB"""
    c = NEAR_FAR
    a_w = 60.0 / 32767.0
    z = fm.fm_station(c["n_wide"], c["Fs_w"], c["weak_f_c"], a_w, c["tone"])
    assert np.all(fm.quantise(z, fm.U8) == 128)
    s16 = fm.quantise(z, fm.S16)
    assert 58 <= int(np.abs(s16.astype(np.int32)).max()) <= 61
    out, clipped = tuned(fmrx, s16, fm.S16, c["weak_f_c"], 0.7 / a_w)
    db = fm.tone_fit_db(out, c["Fs_w"] / c["R"], c["tone"])
    print(f"a station alone at 60 int16 units: tone fit {db:.1f} dB, {clipped} output bytes clamp")
    assert db >= 40.0
    out8, _ = tuned(fmrx, fm.quantise(z, fm.U8), fm.U8, c["weak_f_c"], 0.7 / a_w)
    assert np.all(out8 == 128)


# ---- the int16 RDS capture of tests/test_gpu_tuner_formats_bank.py, decoded on the CPU ---------------------------------
def test_rds_capture_as_int16_decodes_on_the_cpu(oracle):
    """the three-station RDS capture with every amplitude divided by 128, as int16: its u8 quantisation is within +-1 LSB
    of 128; S16 model (gains x 128) -> the oracle's mode-0 discriminator -> rds_oracle.RdsChain -> the station model:
    every station has its PI and PS right from the 20th call to the last"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import rds_oracle
    import _rds_station_model as SM
    import _tuner_formats_capture as FC
    c = TC.RDS
    s16, u8 = FC.rds_capture_s16(also_u8=True)
    assert np.abs(u8.astype(np.int32) - 128).max() <= 1
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    m = fm.TunerModel(h, c["R"], 3, fm.S16)
    for k in range(3):
        m.set_channel(k, c["offsets"][k], c["Fs_w"], FC.rds_gain_s16(k))
    chains = [(oracle.pipeline(0, 1), rds_oracle.RdsChain(upsamp=247, decim=960, sps=26), SM.StationModel(26)) for _ in range(3)]
    step = c["bytes_per_call"] * c["R"]
    right, clipped = [], 0
    for i in range(c["calls"]):
        out = m.process(s16[i * step:(i + 1) * step])
        clipped += int(m.clipped.sum())
        row = []
        for k, (pl, chain, st) in enumerate(chains):
            st.feed_rrc(chain.process(pl.process(out[k])["demod"])["rrc_i"])
            row.append(st.pi == c["pi"][k] and bytes(st.ps).decode("latin-1") == c["ps"][k])
        right.append(row)
    since = [next((i + 1 for i in range(len(right)) if all(r[k] for r in right[i:])), None) for k in range(3)]
    print(f"PI and PS right from calls {since}; tuned bytes clipped: {clipped}")
    assert clipped == 0
    assert all(s is not None and s <= 20 for s in since), f"PI / PS right from calls {since}"
