"""The wideband tuner on the device against its integer model (tests/_tuner_model.py): every output byte and both level
counters EQUAL, for the matrix-core kernel and for the generic kernel, over decimations, filter lengths and channel counts,
with the stream cut into calls of many sizes.  The model is fed the integers fmrx_tuner_design returns (the product's own
host code runs the same function for set_channel), so a libm tie in a tap cannot turn this red; tests/test_tuner_model_host.py
compares those integers with the model's float64 computation."""
import numpy as np
import pytest

import _tuner_model as tm

pytestmark = pytest.mark.gpu

CALLS = (1, 7, 130, 600, 515)        # outputs per channel and call: below a 16-byte piece, a ragged tail, across a 512-output step


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
        gain = (1.0, 0.6, 45.0)[c % 3] * (1.0 + 0.01 * (c % 7))
        plan.append((f_c, gain))
    return plan


def set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain):
    tuner.set_channel(c, f_c, Fs_w, gain)
    model.set_channel_ints(c, *fmrx.Tuner.design(h, Fs_w, f_c, gain))


def same_call(tuner, model, u8, what):
    got, want = tuner.process(u8), model.process(u8)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at channel {bad[0][0]} byte {bad[0][1]}: {got[tuple(bad[0])]} vs model {want[tuple(bad[0])]}"
    cl, pw = tuner.levels()
    assert np.array_equal(cl, model.clipped), f"{what}: clipped counts"
    assert np.array_equal(pw, model.power), f"{what}: power sums"


@pytest.mark.parametrize("N", [1, 7, 70, 200])
@pytest.mark.parametrize("T_of_R", [2, 33, 64, "8R"])
@pytest.mark.parametrize("R", [4, 8, 10, 20])
def test_device_bytes_equal_the_model(fmrx, oracle, variant, R, T_of_R, N):
    T = 8 * R if T_of_R == "8R" else T_of_R
    Fs_w, h = prototype(oracle, R, T)
    rng = np.random.default_rng(1000 * R + 10 * T + N)
    tuner, model = fmrx.Tuner(R, h, N, max(CALLS) * R), tm.TunerModel(h, R, N)
    u8 = rng.integers(0, 256, 2 * R * sum(CALLS), dtype=np.uint8)
    same_call(tuner, model, u8[:2 * R * 40], "default channels (f_c = 0, gain 1)")
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    pos = 0
    for n_out in CALLS:
        same_call(tuner, model, u8[pos:pos + 2 * R * n_out], f"call of {n_out} outputs")
        pos += 2 * R * n_out
    if N >= 3:
        assert model.clipped[2] > 0, "the clipping gain did not clip"
    # set_channel between calls: takes effect at the next call, the other channels and the stream's state untouched
    set_both(fmrx, tuner, model, N - 1, h, Fs_w, -0.2 * Fs_w, 2.0)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.31 * Fs_w, 0.9)
    same_call(tuner, model, u8[:2 * R * 300], "after set_channel")
    # reset: silence in front, counter 0, channels keep their settings
    tuner.reset()
    model.reset()
    same_call(tuner, model, u8[2 * R * 100:2 * R * 700], "after reset")
    tuner.close()


def test_all_zero_and_all_255_input(fmrx, oracle, variant):
    R, T, N = 8, 64, 5
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = fmrx.Tuner(R, h, N, 1024 * R), tm.TunerModel(h, R, N)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, np.random.default_rng(1))):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    same_call(tuner, model, np.zeros(2 * R * 1024, np.uint8), "all 0")
    same_call(tuner, model, np.full(2 * R * 1000, 255, np.uint8), "all 255")
    same_call(tuner, model, np.full(2 * R * 520, 128, np.uint8), "silence")


def test_extreme_gains(fmrx, oracle, variant):
    """scale exponents at both ends of the range: output shifts below 17 (every sample clips) and above 47 (every byte 128)
    take the matrix kernel's 64-bit rounding instead of its 32-bit form"""
    R, T, N = 8, 64, 6
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = fmrx.Tuner(R, h, N, 1100 * R), tm.TunerModel(h, R, N)
    shifts = []
    for c, gain in enumerate((1e6, 1e-5, 3e5, 1.0, 2e8, 1e-8)):
        set_both(fmrx, tuner, model, c, h, Fs_w, (c - 2.5) * 1.1e6, gain)
        shifts.append(model.s[c] + 15)
    assert min(shifts) < 17 and max(shifts) > 47 and 17 <= shifts[3] <= 47
    rng = np.random.default_rng(6)
    same_call(tuner, model, rng.integers(0, 256, 2 * R * 1100, dtype=np.uint8), "extreme gains")
    assert model.clipped[0] > 1000 and model.power[1] == 0


def test_long_filter_runs_the_generic_kernel(fmrx, oracle):
    """more than 256 taps: the matrix kernel does not take the shape, the generic kernel runs whatever the option says"""
    R, T, N = 8, 301, 3
    Fs_w, h = prototype(oracle, R, T)
    tuner, model = fmrx.Tuner(R, h, N, 600 * R), tm.TunerModel(h, R, N)
    rng = np.random.default_rng(2)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain * 0.5)
    for n_out in (5, 600, 77):
        same_call(tuner, model, rng.integers(0, 256, 2 * R * n_out, dtype=np.uint8), f"{n_out} outputs")


def test_phase_counter_wraps_on_the_device(fmrx, oracle, variant):
    """2^32 wide samples = 3.7 minutes at 19.2 MS/s: fed as silence in long calls up to just below the wrap, then a random
    block across it"""
    R, T, N = 32, 16, 2
    Fs_w, h = prototype(oracle, R, T)
    big = (1 << 24) * R                                   # the largest call: 2^29 wide samples = 1 GiB of bytes
    tuner, model = fmrx.Tuner(R, h, N, big), tm.TunerModel(h, R, N)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.123456 * Fs_w, 1.0)
    set_both(fmrx, tuner, model, 1, h, Fs_w, -0.4 * Fs_w, 1.0)
    import torch
    d_wide = torch.full((2 * big,), 128, dtype=torch.uint8, device="cuda")
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
    rng = np.random.default_rng(3)
    same_call(tuner, model, rng.integers(0, 256, 2 * R * 600, dtype=np.uint8), "across 2^32")
    assert model.n == 2 ** 32 + R * 300


def test_destination_pitch_and_channel_offset(fmrx, oracle, variant):
    """process_dev into rows with a pitch larger than the row, two tuners filling disjoint channel ranges of one buffer; what
    lies between the rows is not written"""
    import torch
    R, T = 10, 33
    Fs_w, h = prototype(oracle, R, T)
    n_out, pitch = 700, 1552            # the row is 1400 bytes; the pitch a multiple of 16 above it
    rng = np.random.default_rng(4)
    caps = [rng.integers(0, 256, 2 * R * n_out, dtype=np.uint8) for _ in range(2)]
    counts = (5, 3)
    d_out = torch.full((sum(counts) * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    want, first = [], 0
    keep = []
    for cap, N in zip(caps, counts):
        tuner, model = fmrx.Tuner(R, h, N, n_out * R), tm.TunerModel(h, R, N)
        for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
            set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
        d_wide = torch.from_numpy(cap).cuda()
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


def test_argument_checks(fmrx, oracle):
    Fs_w, h = prototype(oracle, 8, 64)
    E = fmrx.FmrxError
    for R, hh, N, mw in [(1, h, 1, 800), (33, h, 1, 33 * 8), (8, h[:1], 1, 800), (8, h, 0, 800), (8, h, 1, 801), (8, np.zeros(8, np.float32), 1, 800)]:
        with pytest.raises(E):
            fmrx.Tuner(R, hh, N, mw)
    t = fmrx.Tuner(8, h, 2, 800)
    assert t.n_out_bytes(800) == 200 and t.n_out_bytes(801) == 0
    for args in [(2, 0.0, Fs_w, 1.0), (-1, 0.0, Fs_w, 1.0), (0, Fs_w / 2, Fs_w, 1.0), (0, 0.0, Fs_w, float("nan")), (0, 0.0, Fs_w, 0.0)]:
        with pytest.raises(E):
            t.set_channel(*args)
    import torch
    d_wide = torch.zeros(1600 + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(2 * 256 + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w, o = d_wide.data_ptr(), d_out.data_ptr()
    for args in [(w, 801, o, 256), (w, 1600, o, 256), (w, 0, o, 256), (w + 4, 800, o, 256), (w, 800, o + 8, 256), (w, 800, o, 200), (w, 800, o, 192)]:
        with pytest.raises(E):
            t.process_dev(*args)
    t.process_dev(w, 800, o, 208)
    t.levels()
    with pytest.raises(E):
        t.process(np.zeros(2 * 1600, np.uint8))
