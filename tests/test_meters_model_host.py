"""The signal meters' definition (tests/_meters_model.py) against the host-only part of the C ABI (fmrx_meters_table,
fmrx_meters_derive, fmrx_meters_probes) and against closed forms.  No GPU involved."""
import math

import numpy as np
import pytest

import _meters_model as mm


def test_window_sums_to_half_its_length_exactly():
    w = mm.window()
    assert float(w.sum()) == 512.0 and math.fsum(w) == 512.0
    assert w.min() > 0.0 and w.max() < 1.0 and np.abs(w - w[::-1]).max() < 1e-15


def test_probe_frequencies(fmrx):
    assert np.array_equal(fmrx.metersProbes(), np.array(mm.PROBES_HZ))
    assert mm.PROBES_HZ[mm.P_PILOT] == 19000.0
    assert (mm.PROBES_HZ[mm.P_RDS_LO] + mm.PROBES_HZ[mm.P_RDS_HI]) / 2 == 57000.0 and mm.PROBES_HZ[mm.P_RDS_HI] - 57000.0 == 1187.5


@pytest.mark.parametrize("if_Fs", [240000.0, 250000.0])
def test_table_equals_the_model(fmrx, if_Fs):
    """absolute error <= 4 * 2^-53 per entry: what two libms' cos / sin may differ by at |value| <= 1"""
    re, im = fmrx.metersTable(if_Fs)
    want_re, want_im = mm.table(if_Fs)
    assert re.shape == want_re.shape == (5, mm.SEGMENT)
    err = max(float(np.abs(re - want_re).max()), float(np.abs(im - want_im).max()))
    print(f"if_Fs {if_Fs:.0f}: largest difference {err * 2.0 ** 53:.2f} x 2^-53")
    assert err <= 4.0 * 2.0 ** -53


def test_table_rejects_a_rate_whose_top_probe_passes_nyquist(fmrx):
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.metersTable(100000.0)
    assert e.value.code == fmrx.EINVAL


def hand_made_records():
    def rec(**kw):
        r = np.zeros((), mm.METER_DTYPE)
        for k, v in kw.items():
            r[k] = v
        return r
    probe = np.zeros(8)
    probe[:5] = (2.0e-3, 4.0e-3, 50.0, 0.9, 1.1)
    rng = np.random.default_rng(7)
    noise_row = rng.standard_normal(9600).astype(np.float32) * 0.3
    noise_iq = rng.integers(0, 256, 19200, dtype=np.uint8)
    return {
        "all zero": rec(),
        "counts only": rec(n_iq=96000, n_if=9600, segments=9),
        "a station": rec(n_iq=96000, sum_i=-1234, sum_q=987, m2=96000 * 10000, m4=96000 * 100400000, clipped=3, n_if=9600, segments=9,
                         sum_x=12.5, sum_x2=310.0, max_abs=1.9, probe=probe),
        "S = 0: Gaussian moments, M4 = 2 M2^2": rec(n_iq=1000, m2=1000 * 50, m4=1000 * 5000),
        "S = 0: M4 above 2 M2^2": rec(n_iq=1000, m2=1000 * 50, m4=1000 * 9000),
        "M2 - S = 0: constant envelope": rec(n_iq=4096, m2=4096 * 8192, m4=4096 * 8192 * 8192),
        "M2 - S < 0 by rounding": rec(n_iq=3, m2=3 * 8193, m4=3 * 8193 * 8193 - 1),
        "M = 0: sums without segments": rec(n_if=1000, sum_x=-3.0, sum_x2=40.0, max_abs=0.7),
        "noise probes zero, pilot not": rec(n_if=1024, segments=1, probe=np.array([0, 0, 3.0, 0, 0, 0, 0, 0.0])),
        "tiny ratios: below the clamp": rec(n_iq=10, m2=1, m4=1, n_if=1024, segments=1, probe=np.array([1e200, 1e200, 1e-200, 1e-300, 0, 0, 0, 0.0])),
        "huge ratios: above the clamp": rec(n_if=1024, segments=1, probe=np.array([1e-200, 1e-200, 1e200, 1e100, 1e100, 0, 0, 0.0])),
        "full scale and clipped": rec(n_iq=8, sum_i=-1024, sum_q=1016, m2=8 * (128 * 128 + 127 * 127), m4=8 * (128 * 128 + 127 * 127) ** 2, clipped=16),
        "random bytes and a random row": mm.record(noise_iq, noise_row, 240000.0),
    }


@pytest.mark.parametrize("name", list(hand_made_records()))
def test_derive_equals_the_model(fmrx, name):
    r = hand_made_records()[name]
    for if_Fs in (240000.0, 250000.0):
        got, want = fmrx.metersDerive(if_Fs, r), mm.derive(r, if_Fs)
        assert set(got) == set(want) == set(mm.LEVEL_NAMES)
        for k in mm.LEVEL_NAMES:
            assert math.isfinite(got[k]) and math.isfinite(want[k]), (name, k)
            if k.endswith(("_db", "_dbfs")):
                assert mm.DB_MIN <= got[k] <= mm.DB_MAX
                assert abs(got[k] - want[k]) <= 1e-9, (name, k, got[k], want[k])
                if want[k] in (mm.DB_MIN, mm.DB_MAX):
                    assert got[k] == want[k], (name, k)
            else:
                assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (name, k, got[k], want[k])


def test_the_clamps_and_the_empty_cases():
    R = hand_made_records()
    d = mm.derive(R["all zero"], 240000.0)
    assert all(d[k] == mm.DB_MIN for k in ("level_dbfs", "cnr_db", "pilot_db", "rds_db"))
    assert all(d[k] == 0.0 for k in mm.LEVEL_NAMES if not k.endswith(("_db", "_dbfs")))
    assert mm.derive(R["S = 0: Gaussian moments, M4 = 2 M2^2"], 240000.0)["cnr_db"] == mm.DB_MIN
    assert mm.derive(R["S = 0: M4 above 2 M2^2"], 240000.0)["cnr_db"] == mm.DB_MIN
    assert mm.derive(R["M2 - S = 0: constant envelope"], 240000.0)["cnr_db"] == mm.DB_MAX
    assert mm.derive(R["M2 - S < 0 by rounding"], 240000.0)["cnr_db"] == mm.DB_MAX
    d = mm.derive(R["M = 0: sums without segments"], 240000.0)
    assert d["pilot_db"] == mm.DB_MIN and d["rds_db"] == mm.DB_MIN and d["pilot_dev_hz"] == 0.0 and d["freq_offset_hz"] < 0.0
    d = mm.derive(R["noise probes zero, pilot not"], 240000.0)
    assert d["pilot_db"] == mm.DB_MAX and d["rds_db"] == mm.DB_MIN
    d = mm.derive(R["tiny ratios: below the clamp"], 240000.0)
    assert d["pilot_db"] == mm.DB_MIN and d["rds_db"] == mm.DB_MIN
    d = mm.derive(R["huge ratios: above the clamp"], 240000.0)
    assert d["pilot_db"] == mm.DB_MAX and d["rds_db"] == mm.DB_MAX
    d = mm.derive(R["full scale and clipped"], 240000.0)
    assert d["clip_fraction"] == 1.0 and d["dc_i"] == -128.0 and d["dc_q"] == 127.0 and abs(d["level_dbfs"] - 10 * math.log10((16384 + 16129) / 16384)) < 1e-12


def test_rf_group_of_known_bytes():
    g = mm.rf_group(np.array([0, 255, 128, 128, 130, 125, 255, 0], np.uint8))
    assert g == dict(n_iq=4, sum_i=-128 + 0 + 2 + 127, sum_q=127 + 0 - 3 - 128, m2=(16384 + 16129) * 2 + 13,
                     m4=2 * (16384 + 16129) ** 2 + 169, clipped=4)


def test_a_pure_pilot_reads_its_amplitude():
    """x = A cos(2 pi 19000 k / Fs + 0.3), A = 0.1767, four segments: pilot_dev_hz * 2 pi / if_Fs within 1e-3 of A (the
    Hann image at 162 bins leaks below 1e-6 and the window sum is exact), whatever phase a segment starts at."""
    A, Fs = 0.1767, 240000.0
    k = np.arange(4096, dtype=np.float64)
    x = (A * np.cos(2 * np.pi * 19000.0 * k / Fs + 0.3)).astype(np.float32)
    d = mm.derive(mm.record(None, x, Fs), Fs)
    got = d["pilot_dev_hz"] * 2 * np.pi / Fs
    print(f"pilot amplitude {got:.9f} for {A}; pilot_db {d['pilot_db']:.2f}, rds_db {d['rds_db']:.2f}")
    assert abs(got - A) <= 1e-3
    assert d["pilot_db"] > 60.0      # the stated limit: Hann leakage into the noise probes 8.5 bins away
    assert abs(d["peak_dev_hz"] - A * Fs / (2 * np.pi)) < 1.0 and abs(d["freq_offset_hz"]) < 10.0


CNR_DEVIATION_DB = {10.0: 0.04, 20.0: 0.02}   # measured on the inputs below: +0.0324 dB and +0.0101 dB


@pytest.mark.parametrize("cnr", [10.0, 20.0])
def test_m2m4_reads_the_cnr_of_a_carrier_in_noise(cnr):
    """A unit-modulus carrier (uniform random phase) plus complex Gaussian noise at a true CNR of 10 and 20 dB, scaled by 64,
    rounded to integers, n_iq = 2^18, seed 20261019.  Measured on exactly this input: cnr_db = 10.0324 dB and 20.0101 dB, i.e.
    the estimator's variance and the rounding together move it by +0.0324 dB and +0.0101 dB.  Asserted: that deviation (rounded
    up to 0.04 / 0.02 dB) plus 0.5 dB."""
    rng = np.random.default_rng(20261019)
    n = 1 << 18
    ph = rng.uniform(0, 2 * np.pi, n)
    sigma = math.sqrt(10 ** (-cnr / 10) / 2)
    z = np.rint(64 * (np.exp(1j * ph) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))))
    assert np.abs(z.real).max() < 127 and np.abs(z.imag).max() < 127
    u8 = np.empty(2 * n, np.uint8)
    u8[0::2], u8[1::2] = z.real + 128, z.imag + 128
    d = mm.derive(mm.record(u8, None, 240000.0), 240000.0)
    print(f"true CNR {cnr} dB: cnr_db {d['cnr_db']:.4f} (deviation {d['cnr_db'] - cnr:+.4f} dB), level {d['level_dbfs']:.2f} dBFS")
    assert abs(d["cnr_db"] - cnr) <= CNR_DEVIATION_DB[cnr] + 0.5
    assert d["clip_fraction"] == 0.0


def test_the_bank_capture_meets_its_conditions_on_the_cpu_models(oracle):
    """Conditions (b) - (d) of tests/test_gpu_meters_bank.py are properties of the definition and of the capture, not of the
    kernels: here they are on the CPU models (the tuner's integer model, the oracle's front end and discriminator, the
    meters' model), last of the three calls.  Measured: stations against the empty channels' maximum, level_dbfs -1.99 against
    -30.53 dB, cnr_db 27.80 against -11.07, pilot_db 40.62 against 1.36, rds_db 14.88 against -7.46; the mistuned channel
    reads 18 644 Hz more than the tuned one; pilot_dev_hz 3.45 % to 3.59 % below the generator's 0.1 rad per sample."""
    import _meters_capture as MC
    import _tuner_capture as TC
    import _tuner_model as tm
    c = TC.RDS
    wide = MC.capture()
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    model = tm.TunerModel(h, c["R"], 8)
    for k, (f, g) in enumerate(MC.channels()):
        model.set_channel(k, f, c["Fs_w"], g)
    pipes = [oracle.pipeline(0, 2) for _ in range(8)]
    n_wide = MC.BYTES_PER_CALL // 2 * c["R"]
    for i in range(MC.CALLS):
        tuned = model.process(wide[2 * n_wide * i:2 * n_wide * (i + 1)])
        assert not model.clipped.any()
        rows = [pipes[k].process(tuned[k])["demod"] for k in range(8)]
    assert all(np.isfinite(r).all() for r in rows)
    L = [mm.derive(mm.record(tuned[k], rows[k], 240000.0), 240000.0) for k in range(8)]
    for n in ("level_dbfs", "cnr_db", "pilot_db", "rds_db"):
        stations, empty = min(L[k][n] for k in range(3)), max(L[k][n] for k in range(4, 8))
        print(f"{n}: stations at least {stations:.2f}, empty channels at most {empty:.2f}, margin {stations - empty:.2f} dB")
        assert stations > empty
    d = L[3]["freq_offset_hz"] - L[1]["freq_offset_hz"]
    print(f"mistuned by 20 kHz: freq_offset_hz difference {d:.1f}")
    assert 15000.0 <= d <= 25000.0
    rel = [L[k]["pilot_dev_hz"] / (0.1 * 240000.0 / (2 * np.pi)) - 1.0 for k in range(3)]
    print("pilot_dev_hz relative to 0.1 rad: " + ", ".join(f"{r:+.4f}" for r in rel))
    assert all(abs(r) <= 0.056 for r in rel)
