"""Integer model of the wideband tuner (csrc/kernels_tuner.hip, csrc/tuner_host.hpp), in plain numpy.  It does not call
or link the product's host code: it is the second, independent statement of what the tuner computes, and it is the
DEFINITION of the arithmetic -- the device bytes have to equal it (tests/test_gpu_tuner_exact.py).

One wide capture, interleaved u8 I,Q at Fs_w = R * rf_Fs, in; per channel c (centre offset f_c, gain g_c) u8 I,Q at rf_Fs out:

    y_c[m] = Q( g_c * sum_{k<T} h[k] * x[mR - k] * e^{-j 2 pi f_c (mR - k) / Fs_w} ),    x = (u8 - 128) as complex      (*)

computed in the folded form  e^{-j phi_c(mR)} * sum_k (g_c h[k] e^{+j phi_c(k)}) x[mR - k].  Output m of a stream's first
call has x[0] as its newest sample; samples in front of the stream are 0 (raw byte 128).

The arithmetic:
  * h: the prototype low-pass as float32 (the project's filters are), taken to float64.
  * w = llround(f_c / Fs_w * 2^32) mod 2^32 (half away from zero).  Every phase is w * n mod 2^32, n the absolute
    wide-sample index since create / reset, itself taken mod 2^32 (uint32 wrap-around: exact for any stream length).
  * taps, float64:  a_k = 2 pi * ((w k mod 2^32) / 2^32),  g = gain * h[k],  gr = g * cos(a_k),  gi = g * sin(a_k).
  * s: the largest integer with max(|gr|, |gi|) * 2^s <= 127 * 256 = 32512; -14 <= s <= 47 or the channel is rejected.
    (32512, not 32767: a part is split into TWO balanced base-256 digits d0 + 256 d1, each in [-128, 127], for the int8
    matrix cores, and both q and -q have to fit -- the imaginary part meets the Q bytes negated.  It costs < 0.012 bit.)
    re[k] = llround(gr * 2^s), im[k] = llround(gi * 2^s): int16.  Rejected too: non-finite or all-zero gain x taps, and
    128 * sum_k (|re[k]| + |im[k]|) > 2^31 - 1 (the accumulator's worst case).
  * acc = sum_k (re[k] + j im[k]) * x[mR - k], exact in int32:
        ar = sum re[k] xr - im[k] xq,    ai = sum im[k] xr + re[k] xq.
  * rotation: i = (w * (n0 + mR) mod 2^32) >> 20 indexes a 2^12-entry table C[i] = llround(32767 cos(2 pi i / 4096)),
    S[i] = llround(32767 sin(2 pi i / 4096));  yr = ar C + ai S,  yi = ai C - ar S  (acc * (C - jS)), exact in int64.
  * out = clamp(128 + ((y + 2^(s+14)) >> (s+15)), 0, 255), I from yr, Q from yi; >> is the arithmetic shift (floor).
  * levels of a call, per channel: clipped = number of output BYTES whose value was changed by the clamp;
    power = sum over the call's outputs of (I - 128)^2 + (Q - 128)^2 on the clamped bytes.

tuner_f64 is (*) in float64, tuner_bound the distance the integer arithmetic may be from it (derived below, not fitted).
"""
from __future__ import annotations

import numpy as np

TB = 12                      # table bits
LIMIT = 127 * 256            # max |re|, |im|
S_MIN, S_MAX = -14, 47
CHUNK = 1 << 14              # outputs per matmul
M32 = 1 << 32


def llround(v):
    """C llround on float64: half away from zero."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def table():
    i = np.arange(1 << TB)
    a = 2.0 * np.pi * (i / float(1 << TB))
    return llround(32767.0 * np.cos(a)), llround(32767.0 * np.sin(a))


def freq_word(f_c, Fs_w) -> int:
    return int(llround(np.float64(f_c) / np.float64(Fs_w) * 4294967296.0)) % M32


def design_f64(h, Fs_w, f_c, gain):
    """-> (w, s, vr, vi): the frequency word, the scale exponent and the UNROUNDED scaled taps gr 2^s, gi 2^s (float64);
    s is None for a rejected channel."""
    h = np.asarray(h, np.float32).astype(np.float64)
    w = freq_word(f_c, Fs_w)
    k = np.arange(len(h), dtype=np.uint64)
    a = 2.0 * np.pi * (((np.uint64(w) * k) % np.uint64(M32)).astype(np.float64) / 4294967296.0)
    g = np.float64(gain) * h
    gr, gi = g * np.cos(a), g * np.sin(a)
    m = float(max(np.abs(gr).max(), np.abs(gi).max()))
    if not np.isfinite(m) or m == 0.0:
        return w, None, None, None
    s = int(np.floor(np.log2(LIMIT / m)))
    while np.ldexp(m, s) > LIMIT:
        s -= 1
    while np.ldexp(m, s + 1) <= LIMIT:
        s += 1
    if s < S_MIN or s > S_MAX:
        return w, None, None, None
    return w, s, np.ldexp(gr, s), np.ldexp(gi, s)


def design(h, Fs_w, f_c, gain):
    """-> (w, s, re int64[T], im int64[T]); raises ValueError for a channel the tuner rejects."""
    if not (abs(f_c) < Fs_w / 2) or not np.isfinite(gain):
        raise ValueError("f_c / gain out of range")
    w, s, vr, vi = design_f64(h, Fs_w, f_c, gain)
    if s is None:
        raise ValueError("gain x taps rejected")
    re, im = llround(vr), llround(vi)
    if 128 * int(np.abs(re).sum() + np.abs(im).sum()) > 2 ** 31 - 1:
        raise ValueError("accumulator does not fit int32")
    return w, s, re, im


def digits(q):
    """two balanced base-256 digits, least significant first (what the matrix kernel multiplies); q = d0 + 256 d1"""
    q = np.asarray(q, np.int64)
    d0 = ((q + 128) & 255) - 128
    d1 = (q - d0) // 256
    assert np.all(np.abs(q) <= LIMIT) and d1.min() >= -128 and d1.max() <= 127
    return d0, d1


def _windows(xs, T, R, M):
    """xs: int64 samples with T-1 samples of history in front; yields (m_start, W float64[m, T]) with W[j, k] = x[mR - k]."""
    sw = np.lib.stride_tricks.sliding_window_view(xs, T)        # sw[i, t] = xs[i + t]; newest at t = T-1
    for m in range(0, M, CHUNK):
        mm = np.arange(m, min(m + CHUNK, M))
        yield m, sw[mm * R][:, ::-1].astype(np.float64)


def accumulate(u8_wide, hist_u8, re, im, R):
    """acc of N channels: re, im int64[N, T] -> (ar, ai) int64[N, M].  hist_u8: the 2 (T-1) raw bytes in front."""
    re, im = np.atleast_2d(re), np.atleast_2d(im)
    T = re.shape[1]
    u = np.concatenate([np.asarray(hist_u8, np.uint8), np.asarray(u8_wide, np.uint8)]).astype(np.int64) - 128
    assert len(hist_u8) == 2 * (T - 1) and len(u8_wide) % (2 * R) == 0
    xr, xq = u[0::2], u[1::2]
    M = len(u8_wide) // 2 // R
    ar, ai = np.empty((re.shape[0], M), np.int64), np.empty((re.shape[0], M), np.int64)
    fr, fi = re.T.astype(np.float64), im.T.astype(np.float64)     # float64 matmul: every partial sum is an integer < 2^53
    for (m, wr), (_, wq) in zip(_windows(xr, T, R, M), _windows(xq, T, R, M)):
        ar[:, m:m + len(wr)] = np.rint(wr @ fr - wq @ fi).T.astype(np.int64)
        ai[:, m:m + len(wr)] = np.rint(wr @ fi + wq @ fr).T.astype(np.int64)
    assert np.abs(ar).max(initial=0) < 2 ** 31 and np.abs(ai).max(initial=0) < 2 ** 31
    return ar, ai


def rotate_round(ar, ai, w, s, R, n0):
    """one channel: -> (out u8[2M], clipped, power) for outputs whose newest samples are n0, n0 + R, ... (absolute)."""
    ct, st = table()
    M = len(ar)
    n = (np.uint64(n0 % M32) + np.arange(M, dtype=np.uint64) * np.uint64(R)) % np.uint64(M32)
    P = (np.uint64(w) * n) % np.uint64(M32)
    i = (P >> np.uint64(32 - TB)).astype(np.int64)
    c, sn = ct[i], st[i]
    yr, yi = ar * c + ai * sn, ai * c - ar * sn
    sh = s + 15
    o = np.empty(2 * M, np.int64)
    o[0::2] = 128 + ((yr + (1 << (sh - 1))) >> sh)
    o[1::2] = 128 + ((yi + (1 << (sh - 1))) >> sh)
    oc = np.clip(o, 0, 255)
    d = oc - 128
    return oc.astype(np.uint8), int(np.count_nonzero(oc != o)), int((d * d).sum())


class TunerModel:
    """The tuner as a stream: state = the last T-1 wide samples as raw bytes and the sample counter."""

    def __init__(self, h, R, n_channels):
        self.h = np.asarray(h, np.float32)
        self.R, self.T, self.N = int(R), len(self.h), int(n_channels)
        self.w = [0] * self.N
        self.s = [0] * self.N
        self.re = np.zeros((self.N, self.T), np.int64)
        self.im = np.zeros((self.N, self.T), np.int64)
        for c in range(self.N):
            self.set_channel(c, 0.0, 1.0, 1.0)
        self.reset()

    def reset(self):
        self.hist = np.full(2 * (self.T - 1), 128, np.uint8)
        self.n = 0
        self.clipped = np.zeros(self.N, np.uint64)
        self.power = np.zeros(self.N, np.uint64)

    def set_channel(self, c, f_c, Fs_w, gain):
        self.set_channel_ints(c, *design(self.h, Fs_w, f_c, gain))

    def set_channel_ints(self, c, w, s, re, im):
        self.w[c], self.s[c] = int(w), int(s)
        self.re[c], self.im[c] = np.asarray(re, np.int64), np.asarray(im, np.int64)

    def process(self, u8_wide):
        u8_wide = np.asarray(u8_wide, np.uint8)
        ar, ai = accumulate(u8_wide, self.hist, self.re, self.im, self.R)
        out = np.empty((self.N, 2 * ar.shape[1]), np.uint8)
        for c in range(self.N):
            out[c], cl, pw = rotate_round(ar[c], ai[c], self.w[c], self.s[c], self.R, self.n)
            self.clipped[c], self.power[c] = cl, pw
        self.hist = np.concatenate([self.hist, u8_wide])[-2 * (self.T - 1):] if self.T > 1 else self.hist
        self.n += len(u8_wide) // 2
        return out


# --------------------------------------------------------------------------------------------------------------------
# the float64 statement and the bound
# --------------------------------------------------------------------------------------------------------------------
def tuner_f64(u8_wide, hist_u8, h, R, cycles_per_sample, gain, n0=0):
    """(*) in float64: -> complex128[M], the unrounded output in LSB (the byte is 128 + it).  cycles_per_sample = f_c / Fs_w.
    The phase is reduced mod 1 cycle before the cosine, so a large n0 costs little: cps * n is below 2^32 cycles, its float64
    rounding error below 2^-53 * 2^32 = 2^-21 cycles even at the end of the counter (tuner_bound's last term)."""
    h = np.asarray(h, np.float32).astype(np.float64)
    T = len(h)
    u = np.concatenate([np.asarray(hist_u8, np.uint8), np.asarray(u8_wide, np.uint8)]).astype(np.float64) - 128.0
    z = u[0::2] + 1j * u[1::2]
    n = np.float64(n0) - (T - 1) + np.arange(len(z), dtype=np.float64)          # absolute index of z[i]
    z = z * np.exp(-2j * np.pi * np.modf(np.float64(cycles_per_sample) * n)[0])
    M = len(u8_wide) // 2 // R
    sw = np.lib.stride_tricks.sliding_window_view(z, T)
    y = np.empty(M, np.complex128)
    for m in range(0, M, CHUNK):
        mm = np.arange(m, min(m + CHUNK, M))
        y[mm] = sw[mm * R][:, ::-1] @ h
    return np.float64(gain) * y


def tuner_bound(u8_wide, hist_u8, re, im, w, s, R, cycles_per_sample, n0=0):
    """Per output sample, the largest distance (in LSB, I and Q alike) between the model's byte and clip(128 + tuner_f64):

      1/2                                   the final rounding (add half, floor)
    + sqrt(2) 2^-(s+1) sum_k (|xr| + |xq|)  tap rounding: each part of a tap is off by <= 1/2 unit of 2^-s, so each part of
                                            acc 2^-s is off by <= 2^-(s+1) sum (|xr| + |xq|); the rotation turns the error
                                            vector, whose length is at most sqrt(2) times a part
    + |a| (2 pi / 4096 + 2^-15 (1 + 1/sqrt 2))
                                            a = acc 2^-s: the table index drops up to one table step of phase (2 pi / 4096);
                                            each table entry is rounded (vector error <= sqrt(2)/2 units of 1/32768) and the
                                            table is scaled 32767 while the shift divides by 32768 (|a| / 32768)
    + |a| 2 pi |cps - w'/2^32| n            the frequency word's rounding (w' = w as a signed word): a phase drift of that many
                                            cycles per wide sample, n = the output's absolute index (the taps carry the same
                                            quantised frequency, so the folded form drifts as one)
    + |a| 2 pi 2^-21 + 1e-9                 float64's own phase error at n up to 2^32 (2^-53 * 2^32 cycles) and summation noise
    """
    ar, ai = accumulate(u8_wide, hist_u8, re, im, R)
    a = np.hypot(ar[0].astype(np.float64), ai[0].astype(np.float64)) * 2.0 ** -s
    T = np.atleast_2d(re).shape[1]
    u = np.abs(np.concatenate([np.asarray(hist_u8, np.uint8), np.asarray(u8_wide, np.uint8)]).astype(np.float64) - 128.0)
    mag = u[0::2] + u[1::2]
    cs = np.concatenate([[0.0], np.cumsum(mag)])
    M = len(a)
    hi = (T - 1) + np.arange(M) * R + 1                      # one past the newest sample of output m (history-extended index)
    sx = cs[hi] - cs[hi - T]
    wsig = w - M32 if w >= M32 // 2 else w
    n = np.float64(n0) + np.arange(M, dtype=np.float64) * R
    return (0.5 + np.sqrt(2.0) * 2.0 ** -(s + 1) * sx + a * (2 * np.pi / 4096 + 2.0 ** -15 * (1 + np.sqrt(0.5)))
            + a * 2 * np.pi * abs(np.float64(cycles_per_sample) - wsig / 4294967296.0) * n + a * 2 * np.pi * 2.0 ** -21 + 1e-9)
