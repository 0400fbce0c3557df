"""The rational-rate tuner on the device against its integer model (tests/_tuner_rational_model.py): every output byte and
both level counters EQUAL, for the matrix-core kernels and for the generic kernels, for the three input formats, over ratios,
filter lengths and channel counts, with the stream cut into calls of D * {1, 3, 13, 40} wide samples: one period, a partial
tile, a partial 16-byte piece at the row's end.  The model is fed the integers fmrx_tuner_design_rational returns (the
product's own host code runs the same function for set_channel), so a libm tie in a tap cannot turn this red;
tests/test_tuner_rational_model_host.py compares those integers with the model's float64 computation."""
import numpy as np
import pytest

import _tuner_formats_model as fm
import _tuner_model as tm
import _tuner_rational_model as rm

pytestmark = pytest.mark.gpu

PERIODS = (1, 3, 13, 40)             # calls of D * these wide samples = U * these outputs per channel
FMT_NAMES = {fm.U8: "u8", fm.S8: "s8", fm.S16: "s16"}
FORMATS = [fm.U8, fm.S8, fm.S16]
ids = lambda f: FMT_NAMES[f] if isinstance(f, int) and f in FMT_NAMES else None   # noqa: E731


@pytest.fixture(params=["mfma", "generic"])
def variant(request, fmrx):
    fmrx.set_option("tuner_variant", request.param)
    yield request.param
    fmrx.set_option("tuner_variant", "mfma")


def capture_rate(U, D):
    return 10e6 if (U, D) == (18, 125) else 2.4e6 * D / U


def prototype(oracle, U, D, T):
    Fs_w = capture_rate(U, D)
    if T == 2:
        return Fs_w, np.array([0.5, 0.5], np.float32)
    rf_Fs = Fs_w * U / D
    return Fs_w, (np.float32(U) * oracle.impulse_response_lpf(U * Fs_w, 0.5 * (128e3 + rf_Fs - 100e3), T)).astype(np.float32)


def random_raw(rng, n_values, fmt):
    lo, hi = fm.FULL_SCALE[fmt]
    return rng.integers(lo, hi + 1, n_values).astype(fm.DTYPES[fmt])


def channel_plan(N, Fs_w, rng):
    """(f_c, gain) per channel: 0, +-raster, off the raster, next to +-Fs_w/2, then random; every third gain clips"""
    fixed = [0.0, 100e3, -100e3, 1234567.891, Fs_w / 2 - 0.01, -Fs_w / 2 + 0.01, Fs_w / 2 - 3e3, -37.5]
    plan = []
    for c in range(N):
        f_c = fixed[c] if c < len(fixed) else float(rng.uniform(-0.4999, 0.4999) * Fs_w)
        gain = (1.0, 0.6, 45.0)[c % 3] * (1.0 + 0.01 * (c % 7))
        plan.append((f_c, gain))
    return plan


def set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain):
    tuner.set_channel(c, f_c, Fs_w, gain)
    model.set_channel_ints(c, *fmrx.Tuner.design_rational(h, model.U, Fs_w, f_c, gain))


def same_call(tuner, model, values, what):
    got, want = tuner.process(values), model.process(values)
    assert got.shape == want.shape, f"{what}: {got.shape} vs model {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at channel {bad[0][0]} byte {bad[0][1]}: {got[tuple(bad[0])]} vs model {want[tuple(bad[0])]}"
    cl, pw = tuner.levels()
    assert np.array_equal(cl, model.clipped), f"{what}: clipped counts"
    assert np.array_equal(pw, model.power), f"{what}: power sums"


def pair(fmrx, U, D, h, N, max_wide, fmt):
    return fmrx.Tuner.rational(U, D, h, N, max_wide, fmt=FMT_NAMES[fmt]), rm.TunerRationalModel(h, U, D, N, fmt)


@pytest.mark.parametrize("N", [1, 7, 70])
@pytest.mark.parametrize("T_of", [2, "U+1", "8D", "5U+1"])
@pytest.mark.parametrize("U,D", [(2, 5), (3, 10), (6, 25), (18, 125)])
@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_device_bytes_equal_the_model(fmrx, oracle, variant, fmt, U, D, T_of, N):
    T = {2: 2, "U+1": U + 1, "8D": 8 * D, "5U+1": 5 * U + 1}[T_of]
    Fs_w, h = prototype(oracle, U, D, T)
    rng = np.random.default_rng(100000 * fmt + 1000 * D + 10 * T + N)
    tuner, model = pair(fmrx, U, D, h, N, max(PERIODS) * D, fmt)
    assert (tuner.U, tuner.D) == tuner.ratio() == (U, D)
    values = random_raw(rng, 2 * D * sum(PERIODS), fmt)
    same_call(tuner, model, values[:2 * D * 5], "default channels (f_c = 0, gain 1)")
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    pos = 0
    for k in PERIODS:
        same_call(tuner, model, values[pos:pos + 2 * D * k], f"call of {k} periods")
        pos += 2 * D * k
    if N >= 3 and T > 2:
        assert model.clipped[2] > 0, "the clipping gain did not clip"
    # set_channel between calls: takes effect at the next call, the other channels and the stream's state untouched
    set_both(fmrx, tuner, model, N - 1, h, Fs_w, -0.2 * Fs_w, 2.0)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.31 * Fs_w, 0.9)
    same_call(tuner, model, values[:2 * D * 17], "after set_channel")
    # reset: silence in front, counter 0, channels keep their settings
    tuner.reset()
    model.reset()
    same_call(tuner, model, values[2 * D * 3:2 * D * 40], "after reset")
    tuner.close()


@pytest.mark.parametrize("U,D,T", [(2, 5, 40), (6, 25, 200), (18, 125, 1000)])
@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_three_calls_in_a_row_equal_one_long_call(fmrx, oracle, variant, fmt, U, D, T):
    """also the only calls here that span more than one step of the matrix kernel (16 tiles' columns of 8 D wide samples)"""
    N, periods = 5, (530, 9, 131)
    Fs_w, h = prototype(oracle, U, D, T)
    rng = np.random.default_rng(D + fmt)
    values = random_raw(rng, 2 * D * sum(periods), fmt)
    long_t, model = pair(fmrx, U, D, h, N, D * sum(periods), fmt)
    cut_t = fmrx.Tuner.rational(U, D, h, N, D * max(periods), fmt=FMT_NAMES[fmt])
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, long_t, model, c, h, Fs_w, f_c, gain)
        cut_t.set_channel(c, f_c, Fs_w, gain)
    whole = long_t.process(values)
    assert np.array_equal(whole, model.process(values))
    cl, pw = long_t.levels()
    assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power)
    parts, pos = [], 0
    for k in periods:
        parts.append(cut_t.process(values[pos:pos + 2 * D * k]))
        pos += 2 * D * k
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_all_minimum_maximum_and_silence(fmrx, oracle, variant, fmt):
    U, D, T, N = 6, 25, 200, 5
    Fs_w, h = prototype(oracle, U, D, T)
    tuner, model = pair(fmrx, U, D, h, N, 200 * D, fmt)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, np.random.default_rng(1))):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    lo, hi = fm.FULL_SCALE[fmt]
    dt = fm.DTYPES[fmt]
    same_call(tuner, model, np.full(2 * D * 200, lo, dt), "all minimum")
    same_call(tuner, model, np.full(2 * D * 190, hi, dt), "all maximum")
    same_call(tuner, model, np.full(2 * D * 150, 128 if fmt == fm.U8 else 0, dt), "silence")


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_both_ends_of_the_scale_exponent(fmrx, oracle, variant, fmt):
    """output shifts below 17 (every sample clips) and at the top of the format's range (every byte 128) take the matrix
    kernel's 64-bit rounding instead of its 32-bit form; s = -14 and s = 47 (39 for S16) are the ends of the range"""
    U, D, T, N = 3, 10, 80, 6
    Fs_w, h = prototype(oracle, U, D, T)
    by_s = {}
    for e in np.arange(-11.0, 10.0, 0.02):
        w, s, vr, vi = rm.design_f64(h, U, Fs_w, 1.1e6, 10.0 ** e)
        if s is not None:
            by_s.setdefault(s, 10.0 ** e)
    s_top = fm.s_max(fmt)
    tuner, model = pair(fmrx, U, D, h, N, 300 * D, fmt)
    for c, gain in enumerate((by_s[tm.S_MIN], by_s[s_top], 3e5, 1.0, by_s[-10], by_s[s_top - 1])):
        set_both(fmrx, tuner, model, c, h, Fs_w, 1.1e6, gain)
    assert model.s[0] == tm.S_MIN and model.s[1] == s_top
    if s_top < tm.S_MAX:
        with pytest.raises(fmrx.FmrxError):
            tuner.set_channel(2, 1.1e6, Fs_w, by_s[s_top + 1])
    rng = np.random.default_rng(6)
    same_call(tuner, model, random_raw(rng, 2 * D * 300, fmt), "extreme gains")
    assert model.clipped[0] > 1000 and model.power[1] == 0


@pytest.mark.parametrize("U,D,T", [(25, 127, 260), (1, 40, 33), (6, 25, 6 * 257), (32, 511, 100)])
def test_outside_the_matrix_kernels_range_runs_the_generic_kernel(fmrx, oracle, variant, U, D, T):
    """U > 24, D > 125 or Tp > 256: the generic kernel runs whatever the option says; U = 1 with D > 32 is a rational handle"""
    N = 3
    Fs_w = 2.4e6 * D / U
    h = (np.float32(U) * oracle.impulse_response_lpf(U * Fs_w, 1.2e6, T)).astype(np.float32)
    rng = np.random.default_rng(U)
    for fmt in FORMATS:
        tuner, model = pair(fmrx, U, D, h, N, 40 * D, fmt)
        for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
            set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain * 0.5)
        for k in (1, 40, 7):
            same_call(tuner, model, random_raw(rng, 2 * D * k, fmt), f"{FMT_NAMES[fmt]} {k} periods")


def test_phase_counter_wraps_on_the_device(fmrx, oracle, variant):
    """2^32 wide samples: fed as silence in long calls (multiples of D) up to just below the wrap, then a random block across it"""
    U, D, T, N = 3, 100, 16, 2
    Fs_w, h = prototype(oracle, U, D, T)
    big, calls = 50_000_000, 85                           # 1.5e6 outputs per channel and call
    tuner, model = pair(fmrx, U, D, h, N, big, fm.U8)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.123456 * Fs_w, 1.0)
    set_both(fmrx, tuner, model, 1, h, Fs_w, -0.4 * Fs_w, 1.0)
    import torch
    pitch = tuner.n_out_bytes(big)
    assert pitch == 2 * big // D * U and pitch % 16 == 0
    d_wide = torch.full((2 * big,), 128, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(N * pitch, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(calls):                                # 85 * 5e7 samples of silence; the model only moves its counter
        tuner.process_dev(d_wide.data_ptr(), big, d_out.data_ptr(), pitch)
    torch.cuda.synchronize()
    last = 2 ** 32 - calls * big - D * 100 - 96               # 2^32 = 96 mod 100: the stream stands 100 periods and 96 samples below it
    assert last % D == 0 and 0 < last < big
    tuner.process_dev(d_wide.data_ptr(), last, d_out.data_ptr(), pitch)
    torch.cuda.synchronize()
    del d_wide, d_out
    model.n = calls * big + last
    assert model.n == 2 ** 32 - D * 100 - 96
    rng = np.random.default_rng(3)
    same_call(tuner, model, rng.integers(0, 256, 2 * D * 200, dtype=np.uint8), "across 2^32")
    assert model.n > 2 ** 32


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
def test_destination_pitch_larger_than_the_row(fmrx, oracle, variant, fmt):
    """process_dev into rows with a pitch larger than the row; what lies between the rows is not written"""
    import torch
    U, D, T, N, periods = 6, 25, 199, 5, 37
    Fs_w, h = prototype(oracle, U, D, T)
    row, pitch = 2 * U * periods, 480                    # the row is 444 bytes; the pitch a multiple of 16 above it
    rng = np.random.default_rng(4)
    tuner, model = pair(fmrx, U, D, h, N, D * periods, fmt)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    cap = random_raw(rng, 2 * D * periods, fmt)
    d_out = torch.full((N * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    d_wide = torch.from_numpy(cap.view(np.uint8)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert tuner.n_out_bytes(D * periods) == row
    tuner.process_dev(d_wide.data_ptr(), D * periods, d_out.data_ptr(), pitch, stream=stream.cuda_stream)
    want = model.process(cap)
    cl, pw = tuner.levels()
    stream.synchronize()
    assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power)
    got = d_out.cpu().numpy().reshape(N, pitch)
    assert np.array_equal(got[:, :row], want)
    assert np.all(got[:, row:] == 0xA5)


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("R", [4, 10])
def test_u_1_is_the_integer_tuner(fmrx, oracle, variant, R, fmt):
    """Tuner.rational(1, R, ...) and Tuner(R, ...) in one process: bytes and levels"""
    T, N = 8 * R, 5
    Fs_w = 2.4e6 * R
    h = oracle.impulse_response_lpf(Fs_w, 300e3, T)
    a = fmrx.Tuner.rational(1, R, h, N, 700 * R, fmt=FMT_NAMES[fmt])
    b = fmrx.Tuner(R, h, N, 700 * R, fmt=FMT_NAMES[fmt])
    assert a.ratio() == b.ratio() == (1, R) and (a.U, a.D, a.R) == (b.U, b.D, b.R) == (1, R, R)
    rng = np.random.default_rng(R)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        a.set_channel(c, f_c, Fs_w, gain)
        b.set_channel(c, f_c, Fs_w, gain)
    for n_out in (7, 700, 130):
        values = random_raw(rng, 2 * R * n_out, fmt)
        assert np.array_equal(a.process(values), b.process(values))
        (ca, pa), (cb, pb) = a.levels(), b.levels()
        assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
    assert cb[2] > 0


@pytest.mark.parametrize("fmt", FORMATS, ids=ids)
@pytest.mark.parametrize("T", [2, 256])
@pytest.mark.parametrize("D", [32, 33])
def test_both_sides_of_the_integer_kernels_boundary(fmrx, oracle, variant, D, T, fmt):
    """U = 1 with D = 32, the last rate the integer matrix kernels run (T = 256, S16: their largest window, 52,320 bytes of
    LDS), and D = 33, the first that runs the rational ones; three calls on one handle, so history and counter carry"""
    N = 5
    Fs_w, h = prototype(oracle, 1, D, T)
    tuner, model = pair(fmrx, 1, D, h, N, 700 * D, fmt)
    same = fmrx.Tuner(D, h, N, 700 * D, fmt=FMT_NAMES[fmt]) if D == 32 else None
    rng = np.random.default_rng(1000 * D + 10 * T + fmt)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
        if same:
            same.set_channel(c, f_c, Fs_w, gain)
    for n_out in (7, 700, 130):
        values = random_raw(rng, 2 * D * n_out, fmt)
        got, want = tuner.process(values), model.process(values)
        assert np.array_equal(got, want), f"call of {n_out} outputs: bytes differ from the model"
        cl, pw = tuner.levels()
        assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power), f"call of {n_out} outputs: levels"
        if same:
            assert np.array_equal(same.process(values), got), f"call of {n_out} outputs: bytes differ from Tuner({D}, ...)"
        assert model.clipped[2] > 0, "the clipping gain did not clip"


def test_argument_checks(fmrx, oracle):
    Fs_w, h = prototype(oracle, 6, 25, 200)
    E = fmrx.FmrxError
    # gcd, U and D out of range, D < 2 U, max_wide_samples no multiple of D, taps, channels, format
    for U, D, hh, N, mw, word in [(6, 24, h, 1, 2400, "gcd"), (0, 5, h, 1, 500, "U"), (33, 67, h, 1, 6700, "U"), (6, 11, h, 1, 1100, "D"),
                                  (3, 513, h, 1, 5130, "D"), (6, 25, h, 1, 2501, "max_wide_samples"), (6, 25, h[:1], 1, 2500, "taps"),
                                  (6, 25, h, 0, 2500, "n_channels")]:
        with pytest.raises(E, match=word) as e:
            fmrx.Tuner.rational(U, D, hh, N, mw)
        assert e.value.code == fmrx.EINVAL
    with pytest.raises(ValueError):
        fmrx.Tuner.rational(6, 25, h, 1, 2500, fmt="s32")
    h_p = fmrx._vp()
    assert fmrx.lib.fmrx_tuner_create_rational(fmrx.C.byref(h_p), 6, 25, fmrx._f32(h), len(h), 1, 2500, 7, 0) == fmrx.EINVAL
    t = fmrx.Tuner.rational(6, 25, h, 2, 2500)
    assert t.ratio() == (6, 25) and fmrx.Tuner(8, h[:64], 1, 800).ratio() == (1, 8)
    assert t.n_out_bytes(2500) == 1200 and t.n_out_bytes(25) == 12 and t.n_out_bytes(2501) == 0 and t.n_out_bytes(30) == 0
    import torch
    d_wide = torch.zeros(2 * 2500 + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(2 * 1216 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, o = d_wide.data_ptr(), d_out.data_ptr()
    with pytest.raises(E, match="n_wide"):
        t.process_dev(w, 2501, o, 1216)
    for args in [(w, 5000, o, 1216), (w, 0, o, 1216), (w + 4, 2500, o, 1216), (w, 2500, o + 8, 1216), (w, 2500, o, 1210), (w, 2500, o, 1184)]:
        with pytest.raises(E):
            t.process_dev(*args)
    t.process_dev(w, 2500, o, 1216)
    t.levels()
    with pytest.raises(E, match="n_wide"):
        t.process(np.zeros(2 * 30, np.uint8))
