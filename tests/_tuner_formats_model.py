"""Integer model of the wideband tuner's input formats, in plain numpy: tests/_tuner_model.py extended from unsigned 8-bit
captures to signed 8-bit and signed 16-bit ones.  Like that file it neither calls nor links the product's host code, and it
is the DEFINITION of the arithmetic: the device bytes have to equal it (tests/test_gpu_tuner_formats.py).

A wide sample is an (I, Q) pair of raw values; a format says how a raw value becomes the integer x and how many extra bits
B of input scale it carries:

    format   raw array        x                          B    zero sample
    U8 (0)   uint8            u8 - 128                   0    bytes 0x80
    S8 (1)   int8             the int8 value             0    bytes 0x00
    S16 (2)  int16 (LE)       the int16 value            8    bytes 0x00

Everything else is _tuner_model.py's, for every format: the taps and the frequency word, s, the int16 tap pairs and their
limit 127 * 256, the rotation table, the phase w n mod 2^32, the rotation.  What changes:

  * acc = sum_k taps[k] x[mR - k] is exact in 64 bits (about 2^39 for full-scale int16; int32 does not hold it).
  * the rotation is exact in int64: |y| < 2 * 2^39.1 * 2^15 < 2^56.
  * out = clamp(128 + ((y + 2^(s+14+B)) >> (s+15+B)), 0, 255): full scale in maps to full scale out at unity gain.
  * the shift s + 15 + B has to stay in 1 .. 62: an S16 tuner accepts -14 <= s <= 39.
  * levels as before, on the clamped output bytes.

Two identities follow (tests/test_tuner_formats_host.py, and on the device tests/test_gpu_tuner_formats.py):
  1. an S8 tuner fed bytes b equals a U8 tuner fed b ^ 0x80 (the same x, the same B);
  2. an S16 tuner fed (u8 - 128) << 8 equals a U8 tuner fed the u8: acc and y are exactly 256 times as large, the rounding
     constant and the shift move by the same 8 bits, and floor((256 y + 256 h) / (256 d)) = floor((y + h) / d).

tuner_f64 / tuner_bound: the float64 statement with x in input units and the result divided by 2^B, and the distance the
integer arithmetic may be from it (derived below from _tuner_model.tuner_bound's terms, not fitted).
"""
from __future__ import annotations

import numpy as np

import _tuner_model as tm

U8, S8, S16 = 0, 1, 2
NAMES = {U8: "u8", S8: "s8", S16: "s16"}
DTYPES = {U8: np.uint8, S8: np.int8, S16: np.dtype("<i2")}
EXTRA_BITS = {U8: 0, S8: 0, S16: 8}
FULL_SCALE = {U8: (0, 255), S8: (-128, 127), S16: (-32768, 32767)}     # raw values of the most negative / positive x


def s_max(fmt) -> int:
    """the output shift s + 15 + B stays at or below 62"""
    return tm.S_MAX - EXTRA_BITS[fmt]


def raw(values, fmt):
    """raw interleaved I,Q values of the format's dtype (a wrong dtype is an error, not a conversion)"""
    values = np.asarray(values)
    assert values.dtype == DTYPES[fmt], f"{NAMES[fmt]} capture given as {values.dtype}"
    return values.reshape(-1)


def to_x(values, fmt):
    """raw values -> the integers x (int64)"""
    v = raw(values, fmt).astype(np.int64)
    return v - 128 if fmt == U8 else v


def silence(T, fmt):
    """the T - 1 zero samples in front of a stream, as raw values"""
    return np.full(2 * (T - 1), 128 if fmt == U8 else 0, DTYPES[fmt])


def sample_bytes(fmt) -> int:
    """bytes per complex wide sample"""
    return 2 * np.dtype(DTYPES[fmt]).itemsize


def accumulate(values, hist, re, im, R, fmt):
    """acc of N channels: re, im int64[N, T] -> (ar, ai) int64[N, M]; hist: the 2 (T-1) raw values in front.
    float64 matmuls as in _tuner_model.accumulate: every partial sum is an integer below 2^15 * 2 T * 2^15 < 2^53."""
    re, im = np.atleast_2d(re), np.atleast_2d(im)
    T = re.shape[1]
    assert len(hist) == 2 * (T - 1) and len(values) % (2 * R) == 0
    x = np.concatenate([to_x(hist, fmt), to_x(values, fmt)])
    xr, xq = x[0::2], x[1::2]
    M = len(values) // 2 // R
    ar, ai = np.empty((re.shape[0], M), np.int64), np.empty((re.shape[0], M), np.int64)
    fr, fi = re.T.astype(np.float64), im.T.astype(np.float64)
    for (m, wr), (_, wq) in zip(tm._windows(xr, T, R, M), tm._windows(xq, T, R, M)):
        ar[:, m:m + len(wr)] = np.rint(wr @ fr - wq @ fi).T.astype(np.int64)
        ai[:, m:m + len(wr)] = np.rint(wr @ fi + wq @ fr).T.astype(np.int64)
    assert np.abs(ar).max(initial=0) < 2 ** 40 and np.abs(ai).max(initial=0) < 2 ** 40
    return ar, ai


def rotate_round(ar, ai, w, s, R, n0, fmt):
    """one channel -> (out u8[2M], clipped, power): _tuner_model.rotate_round with the shift s + 15 + B"""
    assert 1 <= s + 15 + EXTRA_BITS[fmt] <= 62
    return tm.rotate_round(ar, ai, w, s + EXTRA_BITS[fmt], R, n0)


class TunerModel(tm.TunerModel):
    """The tuner as a stream, for any format: state = the last T-1 wide samples as raw values and the sample counter."""

    def __init__(self, h, R, n_channels, fmt):
        self.fmt = int(fmt)
        assert self.fmt in DTYPES
        super().__init__(h, R, n_channels)

    def reset(self):
        super().reset()
        self.hist = silence(self.T, self.fmt)

    def set_channel_ints(self, c, w, s, re, im):
        if not tm.S_MIN <= int(s) <= s_max(self.fmt):
            raise ValueError(f"scale exponent {s} outside {tm.S_MIN} .. {s_max(self.fmt)}")
        super().set_channel_ints(c, w, s, re, im)

    def process(self, values):
        values = raw(values, self.fmt)
        ar, ai = accumulate(values, self.hist, self.re, self.im, self.R, self.fmt)
        out = np.empty((self.N, 2 * ar.shape[1]), np.uint8)
        for c in range(self.N):
            out[c], cl, pw = rotate_round(ar[c], ai[c], self.w[c], self.s[c], self.R, self.n, self.fmt)
            self.clipped[c], self.power[c] = cl, pw
        if self.T > 1:
            self.hist = np.concatenate([self.hist, values])[-2 * (self.T - 1):]
        self.n += len(values) // 2
        return out


# --------------------------------------------------------------------------------------------------------------------
# the float64 statement and the bound
# --------------------------------------------------------------------------------------------------------------------
def tuner_f64(values, hist, h, R, cycles_per_sample, gain, fmt, n0=0):
    """(*) of _tuner_model.py in float64 with x in input units, divided by 2^B: complex128[M], the unrounded output in LSB.
    The phase is reduced mod 1 cycle before the cosine, as there."""
    h = np.asarray(h, np.float32).astype(np.float64)
    T = len(h)
    x = np.concatenate([to_x(hist, fmt), to_x(values, fmt)]).astype(np.float64)
    z = x[0::2] + 1j * x[1::2]
    n = np.float64(n0) - (T - 1) + np.arange(len(z), dtype=np.float64)
    z = z * np.exp(-2j * np.pi * np.modf(np.float64(cycles_per_sample) * n)[0])
    M = len(values) // 2 // R
    sw = np.lib.stride_tricks.sliding_window_view(z, T)
    y = np.empty(M, np.complex128)
    for m in range(0, M, tm.CHUNK):
        mm = np.arange(m, min(m + tm.CHUNK, M))
        y[mm] = sw[mm * R][:, ::-1] @ h
    return np.float64(gain) * y * 2.0 ** -EXTRA_BITS[fmt]


def tuner_bound(values, hist, re, im, w, s, R, cycles_per_sample, fmt, n0=0):
    """Per output sample, the largest distance (in LSB) between the model's byte and clip(128 + tuner_f64).  The terms are
    _tuner_model.tuner_bound's, each re-derived with x in input units and one output LSB = 2^(s+15+B) units of y, that is
    2^(s+B) units of acc (S = s + B below):

      1/2                                    the final rounding (add half, floor): unchanged, it happens in output LSB
    + sqrt(2) 2^-(S+1) sum_k (|xr| + |xq|)   tap rounding: each part of a tap is off by <= 1/2, so each part of acc by
                                             <= 1/2 sum (|xr| + |xq|) units of acc = 2^-(S+1) sum (...) LSB; the rotation
                                             turns the error vector, at most sqrt(2) times a part.  (x is up to 2^8 times as
                                             large as a byte and an LSB 2^8 times as many units: the term is the same size
                                             relative to full scale.)
    + |a| (2 pi / 4096 + 2^-15 (1 + 1/sqrt 2))   a = acc 2^-S, the output's magnitude in LSB: the table index drops up to one
                                             table step of phase, the table entries are rounded and scaled 32767 / 32768 --
                                             errors relative to |a|, so unchanged
    + |a| 2 pi |cps - w'/2^32| n             the frequency word's rounding: relative to |a| too
    + |a| 2 pi 2^-21 + 1e-9                  float64's own phase error, and its summation noise: the sum's terms h[k] x 2^-B
                                             are, in LSB, no larger than the U8 sum's (|x| 2^-B <= 128 for every format)
    No term comes from the accumulation itself: it is exact in int64 for every format, as it was in int32 for U8."""
    B = EXTRA_BITS[fmt]
    S = s + B
    ar, ai = accumulate(values, hist, re, im, R, fmt)
    a = np.hypot(ar[0].astype(np.float64), ai[0].astype(np.float64)) * 2.0 ** -S
    T = np.atleast_2d(re).shape[1]
    u = np.abs(np.concatenate([to_x(hist, fmt), to_x(values, fmt)]).astype(np.float64))
    mag = u[0::2] + u[1::2]
    cs = np.concatenate([[0.0], np.cumsum(mag)])
    M = len(a)
    hi = (T - 1) + np.arange(M) * R + 1
    sx = cs[hi] - cs[hi - T]
    wsig = w - tm.M32 if w >= tm.M32 // 2 else w
    n = np.float64(n0) + np.arange(M, dtype=np.float64) * R
    return (0.5 + np.sqrt(2.0) * 2.0 ** -(S + 1) * sx + a * (2 * np.pi / 4096 + 2.0 ** -15 * (1 + np.sqrt(0.5)))
            + a * 2 * np.pi * abs(np.float64(cycles_per_sample) - wsig / 4294967296.0) * n + a * 2 * np.pi * 2.0 ** -21 + 1e-9)


# --------------------------------------------------------------------------------------------------------------------
# captures and the audio figure of the near-far tests
# --------------------------------------------------------------------------------------------------------------------
def quantise(z, fmt):
    """complex float capture, 1.0 = full scale -> raw interleaved values: round half up, clamp to the format's range
    (127 / 32767 units per 1.0, as tests/_tuner_capture.py does for u8)"""
    scale = 32767.0 if fmt == S16 else 127.0
    lo, hi = FULL_SCALE[fmt]
    off = 128.0 if fmt == U8 else 0.0
    iq = np.empty(2 * len(z), np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    return np.clip(np.floor(off + scale * iq + 0.5), lo, hi).astype(DTYPES[fmt])


def fm_station(n_wide, Fs_w, f_c, amplitude, f_tone, deviation=75e3):
    """complex128[n_wide]: an FM carrier at f_c, modulated by a sine of f_tone Hz at the given peak deviation"""
    n = np.arange(n_wide, dtype=np.float64)
    phi = 2 * np.pi * f_c * n / Fs_w - deviation / f_tone * np.cos(2 * np.pi * f_tone * n / Fs_w)
    return amplitude * np.exp(1j * phi)


def tone_fit_db(tuned_u8, rf_Fs, f_tone, audio_Fs=48e3, cutoff=15e3):
    """tuned_u8: one channel's I,Q bytes at rf_Fs.  Discriminate (the angle of z[n] conj z[n-1]), low-pass (the mean over
    rf_Fs / audio_Fs samples, then a 63-tap Hann-windowed sinc at `cutoff`), least-squares fit of DC + a sine of f_tone:
    -> 10 log10(power of the fitted sine / power of the residual).  A constant input (no signal at all) gives -inf."""
    z = (tuned_u8[0::2].astype(np.float64) - 128.0) + 1j * (tuned_u8[1::2].astype(np.float64) - 128.0)
    d = np.angle(z[1:] * np.conj(z[:-1]))
    q = int(round(rf_Fs / audio_Fs))
    a = d[:len(d) // q * q].reshape(-1, q).mean(axis=1)
    k = np.arange(63) - 31
    lp = 2 * cutoff / audio_Fs * np.sinc(2 * cutoff / audio_Fs * k) * np.hanning(65)[1:-1]
    a = np.convolve(a, lp / lp.sum(), mode="valid")[32:]            # and drop the tuner's own start-up
    t = np.arange(len(a)) / audio_Fs
    basis = np.stack([np.ones_like(t), np.cos(2 * np.pi * f_tone * t), np.sin(2 * np.pi * f_tone * t)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, a, rcond=None)
    fit = basis[:, 1:] @ coef[1:]
    res = a - basis @ coef
    pf, pr = float(np.mean(fit ** 2)), float(np.mean(res ** 2))
    if pf == 0.0:
        return -np.inf
    return 10 * np.log10(pf / pr) if pr > 0 else np.inf
