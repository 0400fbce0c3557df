"""The wideband tuner's signed 8-bit and 16-bit input formats on the device against their integer model
(tests/_tuner_formats_model.py): every output byte and both level counters EQUAL, for the matrix-core kernels and for the
generic kernels, over decimations, filter lengths and channel counts, with the stream cut into calls of many sizes; and the
two identities that tie the formats to a u8 tuner in the same process.  As in tests/test_gpu_tuner_exact.py the model is fed
the integers fmrx_tuner_design returns."""
import numpy as np
import pytest

import _tuner_formats_model as fm

pytestmark = pytest.mark.gpu

CALLS = (1, 7, 130, 600, 515, 259)   # outputs per channel and call: below a 16-byte piece, ragged tails, across the steps of
                                     # both matrix kernels (512 outputs for 8-bit input, 256 for 16-bit)
FORMATS = [fm.S8, fm.S16]
fmt_ids = [fm.NAMES[f] for f in FORMATS]


@pytest.fixture(params=["mfma", "generic"])
def variant(request, fmrx):
    fmrx.set_option("tuner_variant", request.param)
    yield request.param
    fmrx.set_option("tuner_variant", "mfma")


def prototype(oracle, R, T):
    Fs_w = 2.4e6 * R
    if T == 2:
        return Fs_w, np.array([0.5, 0.5], np.float32)
    return Fs_w, oracle.impulse_response_lpf(Fs_w, 300e3, T)


def channel_plan(N, Fs_w, rng):
    """(f_c, gain) per channel: 0, +-raster, off the raster, next to +-Fs_w/2, then random; every third gain clips"""
    fixed = [0.0, 100e3, -100e3, 1234567.891, Fs_w / 2 - 0.01, -Fs_w / 2 + 0.01, Fs_w / 2 - 3e3, -37.5]
    plan = []
    for c in range(N):
        f_c = fixed[c] if c < len(fixed) else float(rng.uniform(-0.4999, 0.4999) * Fs_w)
        plan.append((f_c, (1.0, 0.6, 45.0)[c % 3] * (1.0 + 0.01 * (c % 7))))
    return plan


def capture(rng, n_values, fmt):
    """random raw values over the whole range, with runs of both full-scale values (-32768 and 32767 for int16) in it"""
    lo, hi = fm.FULL_SCALE[fmt]
    v = rng.integers(lo, hi + 1, n_values).astype(fm.DTYPES[fmt])
    for k, val in enumerate((lo, hi, lo, hi)):
        at = (k + 1) * n_values // 5
        v[at:at + 300 + 37 * k] = val
    return v


def make_pair(fmrx, h, R, N, max_out, fmt):
    return fmrx.Tuner(R, h, N, max_out * R, fmt=fm.NAMES[fmt]), fm.TunerModel(h, R, N, fmt)


def set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain):
    tuner.set_channel(c, f_c, Fs_w, gain)
    model.set_channel_ints(c, *fmrx.Tuner.design(h, Fs_w, f_c, gain))


def same_call(tuner, model, values, what):
    got, want = tuner.process(values), model.process(values)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at channel {bad[0][0]} byte {bad[0][1]}: {got[tuple(bad[0])]} vs model {want[tuple(bad[0])]}"
    cl, pw = tuner.levels()
    assert np.array_equal(cl, model.clipped), f"{what}: clipped counts"
    assert np.array_equal(pw, model.power), f"{what}: power sums"


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
@pytest.mark.parametrize("N", [1, 7, 70, 200])
@pytest.mark.parametrize("T_of_R", [2, 33, 64, "8R"])
@pytest.mark.parametrize("R", [4, 8, 10, 20])
def test_device_bytes_equal_the_model(fmrx, oracle, variant, R, T_of_R, N, fmt):
    T = 8 * R if T_of_R == "8R" else T_of_R
    Fs_w, h = prototype(oracle, R, T)
    rng = np.random.default_rng(100000 * fmt + 1000 * R + 10 * T + N)
    tuner, model = make_pair(fmrx, h, R, N, max(CALLS), fmt)
    assert tuner.sample_bytes == fm.sample_bytes(fmt)
    values = capture(rng, 2 * R * sum(CALLS), fmt)
    same_call(tuner, model, values[:2 * R * 40], "default channels (f_c = 0, gain 1)")
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    pos = 0
    for n_out in CALLS:
        same_call(tuner, model, values[pos:pos + 2 * R * n_out], f"call of {n_out} outputs")
        pos += 2 * R * n_out
    if N >= 3:
        assert model.clipped[2] > 0, "the clipping gain did not clip"
    # set_channel between calls: takes effect at the next call, the other channels and the stream's state untouched
    set_both(fmrx, tuner, model, N - 1, h, Fs_w, -0.2 * Fs_w, 2.0)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.31 * Fs_w, 0.9)
    same_call(tuner, model, values[:2 * R * 300], "after set_channel")
    # reset: zero samples in front, counter 0, channels keep their settings
    tuner.reset()
    model.reset()
    same_call(tuner, model, values[2 * R * 100:2 * R * 700], "after reset")
    tuner.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
def test_full_scale_input_of_both_signs(fmrx, oracle, variant, fmt):
    R, T, N = 8, 64, 5
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = make_pair(fmrx, h, R, N, 1024, fmt)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, np.random.default_rng(1))):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    lo, hi = fm.FULL_SCALE[fmt]
    dt = fm.DTYPES[fmt]
    same_call(tuner, model, np.full(2 * R * 1024, lo, dt), "all minimum")
    same_call(tuner, model, np.full(2 * R * 1000, hi, dt), "all maximum")
    alt = np.full(2 * R * 777, hi, dt)
    alt[1::2] = lo
    same_call(tuner, model, alt, "I maximum, Q minimum")
    same_call(tuner, model, np.zeros(2 * R * 520, dt), "silence")


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
def test_both_ends_of_the_range_of_s(fmrx, oracle, variant, fmt):
    """scale exponents at both ends of the format's range (output shifts 1 and 62), and for S16 the gains beyond it refused
    with FMRX_EINVAL while the channel keeps its settings"""
    R, T, N = 8, 64, 4
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = make_pair(fmrx, h, R, N, 1100, fmt)
    by_s = {}
    for e in np.arange(-9.5, 10.5, 0.05):
        try:
            by_s.setdefault(fmrx.Tuner.design(h, Fs_w, 1e6, 10.0 ** e)[1], 10.0 ** e)
        except fmrx.FmrxError:
            pass
    top = fm.s_max(fmt)
    for c, s in enumerate((-14, top, -13, top - 1)):
        set_both(fmrx, tuner, model, c, h, Fs_w, (c - 1.5) * 1.1e6, by_s[s])
        assert model.s[c] == s
    assert model.s[1] + 15 + fm.EXTRA_BITS[fmt] == 62
    rng = np.random.default_rng(6)
    values = capture(rng, 2 * R * 1100, fmt)
    same_call(tuner, model, values, "extreme gains")
    assert model.clipped[0] > 1000 and model.power[1] == 0
    if fmt == fm.S16:
        for s in (40, 47):
            with pytest.raises(fmrx.FmrxError) as e:
                tuner.set_channel(1, 1e6, Fs_w, by_s[s])
            assert e.value.code == fmrx.EINVAL
        same_call(tuner, model, values[:2 * R * 300], "after the refused set_channel")


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
def test_long_filter_runs_the_generic_kernel(fmrx, oracle, fmt):
    """more than 256 taps: the generic kernel runs whatever the option says"""
    R, T, N = 8, 301, 3
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = make_pair(fmrx, h, R, N, 600, fmt)
    rng = np.random.default_rng(2)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain * 0.5)
    for n_out in (5, 600, 77):
        same_call(tuner, model, capture(rng, 2 * R * n_out, fmt), f"{n_out} outputs")


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
def test_phase_counter_wraps_on_the_device(fmrx, oracle, variant, fmt):
    """2^32 wide samples, fed as silence in long calls up to just below the wrap, then a random block across it"""
    import torch
    R, T, N = 32, 16, 2
    Fs_w, h = prototype(oracle, R, T)
    big = (1 << 24) * R                                   # the largest call: 2^29 wide samples
    tuner, model = make_pair(fmrx, h, R, N, 1 << 24, fmt)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.123456 * Fs_w, 1.0)
    set_both(fmrx, tuner, model, 1, h, Fs_w, -0.4 * Fs_w, 1.0)
    d_wide = torch.zeros(tuner.sample_bytes * big, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(N * (2 * big // R), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(7):                                    # 7 * 2^29 samples of silence; the model only moves its counter
        tuner.process_dev(d_wide.data_ptr(), big, d_out.data_ptr(), 2 * big // R)
    torch.cuda.synchronize()
    last = big - R * 300
    tuner.process_dev(d_wide.data_ptr(), last, d_out.data_ptr(), 2 * big // R)
    torch.cuda.synchronize()
    del d_wide, d_out
    model.n = 7 * big + last
    assert model.n == 2 ** 32 - R * 300
    same_call(tuner, model, capture(np.random.default_rng(3), 2 * R * 600, fmt), "across 2^32")
    assert model.n == 2 ** 32 + R * 300


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_ids)
def test_destination_pitch_and_channel_offset(fmrx, oracle, variant, fmt):
    """process_dev into rows with a pitch larger than the row, two tuners filling disjoint channel ranges of one buffer; what
    lies between the rows is not written"""
    import torch
    R, T = 10, 33
    Fs_w, h = prototype(oracle, R, T)
    n_out, pitch = 700, 1552            # the row is 1400 bytes; the pitch a multiple of 16 above it
    rng = np.random.default_rng(4)
    caps = [capture(rng, 2 * R * n_out, fmt) for _ in range(2)]
    counts = (5, 3)
    d_out = torch.full((sum(counts) * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    want, first, keep = [], 0, []
    for cap, N in zip(caps, counts):
        tuner, model = make_pair(fmrx, h, R, N, n_out, fmt)
        for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
            set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
        d_wide = torch.from_numpy(cap.view(np.uint8)).cuda()
        assert d_wide.numel() == tuner.sample_bytes * n_out * R
        torch.cuda.synchronize()
        tuner.process_dev(d_wide.data_ptr(), n_out * R, d_out.data_ptr() + first * pitch, pitch, stream=stream.cuda_stream)
        want.append(model.process(cap))
        cl, pw = tuner.levels()
        assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power)
        first += N
        keep.append((tuner, d_wide))
    stream.synchronize()
    got = d_out.cpu().numpy().reshape(sum(counts), pitch)
    assert np.array_equal(got[:, :2 * n_out], np.concatenate(want))
    assert np.all(got[:, 2 * n_out:] == 0xA5)


# ---- the identities, against a u8 tuner in the same process -------------------------------------------------------------
@pytest.mark.parametrize("R,T,N", [(8, 64, 13), (10, 33, 5), (4, 32, 70)])
def test_identities_hold_on_the_device(fmrx, oracle, variant, R, T, N):
    """an S8 tuner fed b ^ 0x80 and an S16 tuner fed (u8 - 128) << 8 equal a U8 tuner fed the u8, byte for byte, levels included"""
    Fs_w, h = prototype(oracle, R, T)
    rng = np.random.default_rng(R + N)
    tuners = {f: fmrx.Tuner(R, h, N, 700 * R, fmt=f) for f in ("u8", "s8", "s16")}
    assert [tuners[f].sample_bytes for f in ("u8", "s8", "s16")] == [2, 2, 4]
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        for t in tuners.values():
            t.set_channel(c, f_c, Fs_w, gain)
    clipped = 0
    for n_out in (3, 700, 129, 512):
        u8 = rng.integers(0, 256, 2 * R * n_out, dtype=np.uint8)
        feeds = {"u8": u8, "s8": (u8 ^ 0x80).view(np.int8), "s16": ((u8.astype(np.int32) - 128) << 8).astype(np.int16)}
        got = {f: (tuners[f].process(feeds[f]), *tuners[f].levels()) for f in tuners}
        for f in ("s8", "s16"):
            for a, b, what in zip(got[f], got["u8"], ("bytes", "clipped", "power")):
                assert np.array_equal(a, b), f"{f} against u8, call of {n_out}: {what}"
        clipped += int(got["u8"][1].sum())
    assert clipped > 0 or N < 3


def test_arguments_of_the_formats(fmrx, oracle):
    Fs_w, h = prototype(oracle, 8, 64)
    with pytest.raises(ValueError):
        fmrx.Tuner(8, h, 1, 800, fmt="s32")
    import ctypes as C
    handle = C.c_void_p()
    for bad in (-1, 3, 16):
        assert fmrx.lib.fmrx_tuner_create_ex(C.byref(handle), 8, np.ascontiguousarray(h, np.float32), len(h), 1, 800, bad, 0) == fmrx.EINVAL
    for f, dtype, other in [("u8", np.uint8, np.int8), ("s8", np.int8, np.uint8), ("s16", np.int16, np.uint8)]:
        t = fmrx.Tuner(8, h, 2, 800, fmt=f)
        assert fmrx.lib.fmrx_tuner_format(t._h) == fmrx.TUNER_FORMATS[f]
        assert t.sample_bytes == 2 * np.dtype(dtype).itemsize and t.n_out_bytes(800) == 200
        assert t.process(np.zeros(1600, dtype)).shape == (2, 200)
        with pytest.raises(TypeError):
            t.process(np.zeros(1600, other))
        with pytest.raises(fmrx.FmrxError):
            t.process(np.zeros(2 * 1600, dtype))
        t.close()
