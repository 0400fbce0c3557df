"""The wideband tuner's integer model (tests/_tuner_model.py) against the float64 statement of the same mathematics, the
host-only part of the C ABI (fmrx_tuner_design / fmrx_tuner_table) against the model's own float64 computation, and the
properties tests/test_gpu_tuner_exact.py and test_gpu_tuner_bank.py build on: cut invariance, the phase counter's wrap,
levels, selectivity through the CPU oracle's mono chain, and the RDS capture of the bank test decoded on the CPU.
No GPU involved."""
import os
import sys

import numpy as np
import pytest

import _rds_station_model as SM
import _tuner_capture as TC
import _tuner_model as tm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rds_oracle  # noqa: E402


def silence(T):
    return np.full(2 * (T - 1), 128, np.uint8)


def check_against_f64(u8, hist, h, R, Fs_w, f_c, gain, n0=0, cps=None):
    """model bytes vs clip(128 + tuner_f64) sample by sample; returns (largest error, smallest margin, clipped)."""
    w, s, re, im = tm.design(h, Fs_w, f_c, gain)
    cps = f_c / Fs_w if cps is None else cps
    ar, ai = tm.accumulate(u8, hist, re, im, R)
    out, clipped, power = tm.rotate_round(ar[0], ai[0], w, s, R, n0)
    y = tm.tuner_f64(u8, hist, h, R, cps, gain, n0)
    b = np.repeat(tm.tuner_bound(u8, hist, re, im, w, s, R, cps, n0), 2)
    want = np.empty(2 * len(y))
    want[0::2], want[1::2] = 128.0 + y.real, 128.0 + y.imag
    d = np.abs(out.astype(np.float64) - np.clip(want, 0.0, 255.0))
    worst = int(np.argmax(d - b))
    assert np.all(d <= b), f"byte {worst}: model {out[worst]} vs float64 {want[worst]:.6f}, bound {b[worst]:.4f}"
    d2 = out.astype(np.int64) - 128
    assert power == int((d2 * d2).sum())
    return float(d.max()), float((b - d).min()), clipped


@pytest.mark.parametrize("R", [4, 8, 10, 20])
def test_model_within_the_derived_bound_of_float64(oracle, R):
    Fs_w, T = 2.4e6 * R, 8 * R + 1
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T)
    rng = np.random.default_rng(R)
    inputs = {"random": rng.integers(0, 256, 2 * R * 3000, dtype=np.uint8), "all 0": np.zeros(2 * R * 500, np.uint8),
              "all 255": np.full(2 * R * 500, 255, np.uint8)}
    for name, u8 in inputs.items():
        for f_c, gain in [(0.0, 0.9), (0.31e6 * R, 0.9), (-1.05e6 * R, 3.0), (-1.19e6 * R, 40.0)]:
            err, margin, clipped = check_against_f64(u8, silence(T), h, R, Fs_w, f_c, gain)
            print(f"R={R} {name} f_c={f_c:+.0f} gain={gain}: max error {err:.4f} LSB, margin {margin:.4f}, clipped {clipped}")


@pytest.fixture(scope="module")
def tones(oracle):
    c = TC.TONES
    n_wide = 4 * 51200 * c["R"]
    return TC.tone_capture(n_wide), oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])


def test_three_station_capture_within_bound_and_unclipped(tones):
    c = TC.TONES
    u8, h = tones
    u8 = u8[:2 * c["R"] * 51200]
    assert u8.min() > 0 and u8.max() < 255
    for f_c, a in zip(c["offsets"], c["amplitudes"]):
        err, margin, clipped = check_against_f64(u8, silence(c["T"]), h, c["R"], c["Fs_w"], f_c, 0.8 / a)
        print(f"f_c={f_c:+.0f}: max error {err:.4f} LSB (margin {margin:.4f}), clipped {clipped}")
        assert clipped == 0
        assert err < 1.0


def test_selectivity_through_the_oracle_mono_chain(tones, oracle):
    """each station's tuned bytes, demodulated by the CPU oracle's mode-0 mono chain, carry that station's tone"""
    c = TC.TONES
    u8, h = tones
    m = tm.TunerModel(h, c["R"], 3)
    for k in range(3):
        m.set_channel(k, c["offsets"][k], c["Fs_w"], 0.8 / c["amplitudes"][k])
    out = m.process(u8)
    assert not m.clipped.any()
    for k in range(3):
        pl = oracle.pipeline(0, 1)
        audio = np.concatenate([pl.process(out[k, i:i + 102400])["audio"] for i in range(0, out.shape[1], 102400)])
        a = audio[1024:].astype(np.float64)
        spec = np.abs(np.fft.rfft((a - a.mean()) * np.hanning(len(a))))
        peak = np.fft.rfftfreq(len(a), 1 / 48e3)[int(np.argmax(spec))]
        assert abs(peak - c["tones"][k]) < 48e3 / len(a) * 1.5, f"station {k}: spectral peak at {peak:.1f} Hz, tone {c['tones'][k]} Hz"


# ---- the host-only ABI against the model's float64 computation ---------------------------------------------------------
def same_or_tie(got, v):
    """got int16[T] equals llround(v), except by one unit where v is within 1e-9 of a half-integer (a libm tie)"""
    want = tm.llround(v)
    diff = got.astype(np.int64) - want
    frac = np.abs(v) - np.floor(np.abs(v))
    ok = (diff == 0) | ((np.abs(diff) == 1) & (np.abs(frac - 0.5) < 1e-9))
    return bool(ok.all())


def test_design_equals_the_model(fmrx, oracle):
    rng = np.random.default_rng(7)
    n = 0
    for R, T in [(4, 2), (4, 33), (8, 64), (10, 80), (20, 160), (32, 256), (8, 301)]:
        Fs_w = 2.4e6 * R
        h = oracle.impulse_response_lpf(Fs_w, 400e3, T) if T > 2 else np.array([0.5, 0.5], np.float32)
        cases = [(0.0, 1.0), (100e3, 1.0), (-100e3, 2.5), (Fs_w / 2 - 1.0, 1.0), (-Fs_w / 2 + 1.0, 0.3), (123456.789, 1e-3), (-7.0, 1e4)]
        cases += [(float(rng.uniform(-0.499, 0.499) * Fs_w), float(10 ** rng.uniform(-3, 3))) for _ in range(12)]
        for f_c, gain in cases:
            w, s, re, im = fmrx.Tuner.design(h, Fs_w, f_c, gain)
            mw, ms, vr, vi = tm.design_f64(h, Fs_w, f_c, gain)
            assert w == mw, f"frequency word, f_c={f_c}"
            assert s == ms, f"scale exponent, f_c={f_c} gain={gain}"
            assert same_or_tie(re, vr) and same_or_tie(im, vi), f"taps, R={R} T={T} f_c={f_c} gain={gain}"
            assert max(np.abs(re).max(), np.abs(im).max()) <= tm.LIMIT
            tm.digits(re), tm.digits(-im.astype(np.int64))
            n += 1
    assert n == 7 * 19


def test_frequency_words():
    assert tm.freq_word(0.0, 19.2e6) == 0
    assert tm.freq_word(4.8e6, 19.2e6) == 1 << 30
    assert tm.freq_word(-4.8e6, 19.2e6) == 3 << 30
    assert tm.freq_word(-1.0, 2.0 ** 32) == 2 ** 32 - 1


def test_table_equals_the_model(fmrx):
    c, s = fmrx.Tuner.table()
    ct, st = tm.table()
    assert len(c) == 1 << tm.TB and np.array_equal(c, ct) and np.array_equal(s, st)
    assert c[0] == 32767 and s[1024] == 32767 and c[2048] == -32767 and s[3072] == -32767 and s[0] == 0 and c[1024] == 0


def test_design_rejects_what_the_model_rejects(fmrx):
    h = np.hanning(34)[1:-1].astype(np.float32)
    bad = [(np.zeros(32, np.float32), 1e6, 0.0, 1.0), (h, 1e6, 0.0, 0.0), (h, 1e6, 0.5e6, 1.0), (h, 1e6, -0.5e6, 1.0), (h, 1e6, 0.0, float("nan")),
           (h, 1e6, 0.0, float("inf")), (h, 1e6, 0.0, 1e-30), (h, 1e6, 0.0, 1e30), (np.ones(1000, np.float32), 1e6, 0.123e6, 1.0)]
    hn = h.copy()
    hn[3] = np.nan
    bad.append((hn, 1e6, 0.0, 1.0))
    for hh, Fs_w, f_c, gain in bad:
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.Tuner.design(hh, Fs_w, f_c, gain)
        assert e.value.code == fmrx.EINVAL
        with pytest.raises(ValueError):
            tm.design(hh, Fs_w, f_c, gain)
    # the int32 worst case is only reachable with long filters: 256 taps of any shape pass
    w, s, re, im = fmrx.Tuner.design(np.ones(256, np.float32), 1e6, 0.123e6, 1.0)
    assert 128 * int(np.abs(re.astype(np.int64)).sum() + np.abs(im.astype(np.int64)).sum()) < 2 ** 31


# ---- properties of the model the device tests rely on ------------------------------------------------------------------
def make_model(oracle, R=10, T=33, N=3):
    Fs_w = 2.4e6 * R
    m = tm.TunerModel(oracle.impulse_response_lpf(Fs_w, 300e3, T), R, N)
    for c, (f_c, g) in enumerate([(0.0, 1.0), (0.9e6 * R, 2.0), (-1.1e6 * R, 0.7)][:N]):
        m.set_channel(c, f_c, Fs_w, g)
    return m


def test_cut_invariance(oracle):
    rng = np.random.default_rng(5)
    R = 10
    u8 = rng.integers(0, 256, 2 * R * 700, dtype=np.uint8)
    whole = make_model(oracle).process(u8)
    m = make_model(oracle)
    parts, pos = [], 0
    for n_out in (1, 2, 7, 64, 300, 326):
        parts.append(m.process(u8[pos:pos + 2 * R * n_out]))
        pos += 2 * R * n_out
    assert pos == len(u8)
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_phase_counter_wraps(oracle):
    """a stream that crosses 2^32 wide samples: the cut at the wrap changes nothing, and the bytes stay within the bound of
    the float64 formula evaluated at the true (unwrapped) sample index"""
    rng = np.random.default_rng(9)
    R, T = 8, 64
    Fs_w = 19.2e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    u8 = rng.integers(64, 192, 2 * R * 400, dtype=np.uint8)
    n0 = 2 ** 32 - R * 200
    a, b = tm.TunerModel(h, R, 1), tm.TunerModel(h, R, 1)
    for m in (a, b):
        m.set_channel(0, 5.2e6, Fs_w, 1.5)
        m.n = n0
    whole = a.process(u8)
    cut = np.concatenate([b.process(u8[:2 * R * 200]), b.process(u8[2 * R * 200:])], axis=1)
    assert b.n == 2 ** 32 + R * 200 and np.array_equal(whole, cut)
    w = a.w[0]
    wsig = w - 2 ** 32 if w >= 2 ** 31 else w
    check_against_f64(u8, silence(T), h, R, Fs_w, 5.2e6, 1.5, n0=n0, cps=wsig / 2.0 ** 32)
    c = tm.TunerModel(h, R, 1)
    c.set_channel(0, 5.2e6, Fs_w, 1.5)
    assert not np.array_equal(c.process(u8), whole)        # the counter matters


def test_saturation_is_counted_in_levels(oracle):
    rng = np.random.default_rng(11)
    R, T, Fs_w = 4, 32, 9.6e6
    h = oracle.impulse_response_lpf(Fs_w, 600e3, T)
    u8 = rng.integers(0, 256, 2 * R * 2000, dtype=np.uint8)
    m = tm.TunerModel(h, R, 2)
    m.set_channel(0, 0.0, Fs_w, 0.5)
    m.set_channel(1, 0.0, Fs_w, 60.0)
    out = m.process(u8)
    assert m.clipped[0] == 0 and m.clipped[1] > 100
    y = tm.tuner_f64(u8, silence(T), h, R, 0.0, 60.0)
    want = np.empty(2 * len(y))
    want[0::2], want[1::2] = 128 + y.real, 128 + y.imag
    sure = int(np.count_nonzero((want < -1.0) | (want > 256.0)))
    maybe = int(np.count_nonzero((want < 0.5) | (want > 254.5)))
    assert sure <= m.clipped[1] <= maybe
    sat = (want < -1.0) | (want > 256.0)
    assert set(np.unique(out[1][sat])) <= {0, 255}
    for c in range(2):
        d = out[c].astype(np.int64) - 128
        assert m.power[c] == (d * d).sum()


# ---- the RDS capture of tests/test_gpu_tuner_bank.py, decoded on the CPU -----------------------------------------------
def test_rds_capture_decodes_on_the_cpu(oracle):
    """integer tuner model -> the oracle's mode-0 discriminator -> rds_oracle.RdsChain -> the station model: station 1 of the
    capture has its PI and PS right from the 20th call to the last (what the GPU test requires of every station)"""
    c = TC.RDS
    k = 1
    u8 = TC.rds_capture()
    assert u8.min() > 0 and u8.max() < 255
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    m = tm.TunerModel(h, c["R"], 1)
    m.set_channel(0, c["offsets"][k], c["Fs_w"], TC.rds_gain(k))
    pl, chain, st = oracle.pipeline(0, 1), rds_oracle.RdsChain(upsamp=247, decim=960, sps=26), SM.StationModel(26)
    step = c["bytes_per_call"] * c["R"]
    right, clipped = [], 0
    for i in range(c["calls"]):
        tuned = m.process(u8[i * step:(i + 1) * step])[0]
        clipped += int(m.clipped[0])
        st.feed_rrc(chain.process(pl.process(tuned)["demod"])["rrc_i"])
        right.append(st.pi == c["pi"][k] and bytes(st.ps).decode("latin-1") == c["ps"][k])
    first = next((i + 1 for i in range(len(right)) if all(right[i:])), None)
    print(f"station {k}: PI and PS right from call {first} on; {st.good} of {st.blocks} blocks pass; tuned bytes clipped: {clipped}")
    assert clipped == 0
    assert first is not None and first <= 20, f"PI / PS right from call {first}"
