"""The de-emphasis filter's definition on the host (no GPU): fmrx_deemph_design against the formula, the float32 model
(tests/_deemph_model.py) against float64, its frequency response, and the speculate / verify / repair walk against the
serial one -- the same bits, and the miss counts of DESIGN.md 4.10."""
import math

import numpy as np
import pytest

import _deemph_model as m

F32, F64 = np.float32, np.float64
FS = 48000.0
SHAPES = [(8, 16), (64, 64), (128, 128), (256, 256), (384, 256)]
# misses of the model's walk at 75 us on the fixed inputs, per (W, L) above, of 255, 63, 31, 15, 15 checked segments
MISSES = {"audio": [255, 18, 0, 0, 0], "audio->silence": [112, 12, 2, 1, 0], "impulse": [254, 13, 2, 1, 0]}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def inputs():
    return m.fixed_inputs()


@pytest.mark.parametrize("fs", [40000.0, 44100.0, 48000.0])
@pytest.mark.parametrize("tau", [50.0, 75.0])
def test_design_equals_the_formula(fmrx, fs, tau):
    """Both sides: glibc's tan and IEEE double operations in one order -> the same float32 bits."""
    p, b0 = fmrx.deemphasisCoeffs(fs, tau)
    wp, wb = m.design(fs, tau)
    assert bits(p) == bits(wp) and bits(b0) == bits(wb)
    assert 0.0 < p < 1.0


def test_design_quoted_values(fmrx):
    assert [f"{v:.8f}" for v in fmrx.deemphasisCoeffs(48000, 75)] == ["0.75471091", "0.12264455"]
    assert [f"{v:.8f}" for v in fmrx.deemphasisCoeffs(48000, 50)] == ["0.65098143", "0.17450930"]


def test_design_rejects(fmrx):
    import ctypes as C
    p, b0 = C.c_float(0), C.c_float(0)
    d = fmrx.lib.fmrx_deemph_design
    assert d(48000.0, 75.0, C.byref(p), C.byref(b0)) == fmrx.OK
    for fs, tau in [(48000.0, 0.0), (48000.0, -75.0), (0.0, 75.0), (-1.0, 75.0), (float("nan"), 75.0), (48000.0, float("nan"))]:
        assert d(fs, tau, C.byref(p), C.byref(b0)) == fmrx.EINVAL, (fs, tau)
        assert m.design(fs, tau) is None
    # 1 / (2 fs tau) >= pi / 4: at tau = 75 us that is fs <= 8488.26...
    edge = 1.0 / (2.0 * 75e-6 * (math.pi / 4))
    assert d(edge * 0.999, 75.0, C.byref(p), C.byref(b0)) == fmrx.EINVAL
    assert d(edge * 1.001, 75.0, C.byref(p), C.byref(b0)) == fmrx.OK and 0.0 < p.value < 1e-2
    assert d(48000.0, 75.0, None, C.byref(b0)) == fmrx.EINVAL
    assert d(48000.0, 75.0, C.byref(p), None) == fmrx.EINVAL


@pytest.mark.parametrize("tau", [50.0, 75.0])
def test_model_against_float64(inputs, tau):
    """The same recurrence in float64 with the same (float32) coefficients.  Per step the float32 walk commits three roundings:
    u (relative 2^-24 of |u| <= 2 X), v = b0 u (2^-24 of |v| <= 2 b0 X) and y (2^-24 of |y| <= Y), i.e. at most
    e = 2^-24 (2 b0 X + 2 b0 X + Y) in y, X = max |x|, Y = max |y| <= X (DC gain 1, |y| <= 2 b0 X / (1 - p) = X).  The error
    obeys err[n] = p err[n-1] + e[n]: a geometric sum, |err| <= e / (1 - p).  (The flush changes nothing above 2^-126.)"""
    p, b0 = m.design(FS, tau)
    x = inputs["audio"]
    y32, _ = m.serial(x, p, b0)
    y64 = np.zeros(len(x), F64)
    xp = yp = 0.0
    for i, v in enumerate(x.astype(F64)):
        yp = float(p) * yp + float(b0) * (v + xp)
        xp = v
        y64[i] = yp
    X = float(np.abs(x).max())
    bound = 2.0 ** -24 * (4.0 * float(b0) * X + X) / (1.0 - float(p))
    err = float(np.abs(y32[0].astype(F64) - y64).max())
    print(f"tau {tau}: max |float32 - float64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("tau", [50.0, 75.0])
def test_frequency_response(tau):
    """Steady-state gain of a float64 run = |b0 (1 + e^-jw) / (1 - p e^-jw)|; the deviation from the analog filter is printed."""
    p, b0 = (float(v) for v in m.design(FS, tau))
    n = 9600
    for f in (1e3, 5e3, 10e3, 15e3):
        w = 2 * math.pi * f / FS
        x = np.exp(1j * w * np.arange(n))
        y = np.zeros(n, complex)
        xp = yp = 0j
        for i in range(n):
            yp = p * yp + b0 * (x[i] + xp)
            xp = x[i]
            y[i] = yp
        gain = abs(y[-1])                     # |x| = 1; the transient has decayed by p^9600
        want = abs(b0 * (1 + np.exp(-1j * w)) / (1 - p * np.exp(-1j * w)))
        analog = 1.0 / math.sqrt(1.0 + (2 * math.pi * f * tau * 1e-6) ** 2)
        print(f"tau {tau} us, {f / 1e3:.0f} kHz: gain {20 * math.log10(gain):+.3f} dB, analog {20 * math.log10(analog):+.3f} dB, "
              f"deviation {20 * math.log10(gain / analog):+.3f} dB")
        assert abs(gain - want) <= 1e-12
    assert abs(b0 * 2 / (1 - p) - 1.0) < 1e-7   # DC gain 1 (up to the float32 rounding of p and b0)


@pytest.mark.parametrize("name", ["audio", "audio->silence", "impulse"])
def test_parallel_walk_equals_serial(inputs, name):
    """Bit for bit, with the carried state, for every shape; and the miss counts at 75 us."""
    x = inputs[name]
    for tau in (50.0, 75.0):
        p, b0 = m.design(FS, tau)
        ys, ss = m.serial(x, p, b0)
        for k, (W, L) in enumerate(SHAPES):
            y, s, missed, segs = m.parallel(x, p, b0, None, W, L)
            assert np.array_equal(bits(y), bits(ys)) and np.array_equal(bits(s), bits(ss)), (name, tau, W, L)
            assert segs == (len(x) + L - 1) // L - 1
            if tau == 75.0:
                print(f"{name} (W, L) = ({W}, {L}): {missed} of {segs}")
                assert missed == MISSES[name][k], (name, W, L)
    assert MISSES[name][0] > 0
    assert (m.BUILTIN_W, m.BUILTIN_L) == SHAPES[3] and MISSES["audio"][3] == 0


def test_parallel_walk_in_unequal_calls(inputs):
    """A stream cut into calls of unequal length, state carried, rows side by side: the serial walk of the whole."""
    p, b0 = m.design(FS, 75.0)
    x = np.stack([inputs["audio"], inputs["audio->silence"], inputs["impulse"]])
    ys, ss = m.serial(x, p, b0)
    for W, L in [(8, 16), (256, 256)]:
        st, at, out = None, 0, []
        for n in (1, 17, L, 1000, 2, 4096):
            y, st, _, _ = m.parallel(x[:, at:at + n], p, b0, st, W, L)
            out.append(y)
            at += n
        y = np.concatenate(out, axis=1)
        assert np.array_equal(bits(y), bits(ys[:, :y.shape[1]]))
        assert np.array_equal(bits(st), bits(ss))


def test_flush_is_needed():
    """Without the flush a state in digital silence sticks at the smallest subnormal: RN(p * 2^-149) = 2^-149."""
    p, _ = m.design(FS, 75.0)
    from _fir_model import fmaf
    tiny = F32(2.0 ** -149)
    assert bits(fmaf(p, tiny, F32(0.0))) == bits(tiny)
    assert bits(m.step(F32(0.0), F32(0.0), tiny, p, F32(0.1))) == bits(F32(0.0))
