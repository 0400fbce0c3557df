"""Integer model of the wideband tuner at a rational rate U/D, in plain numpy: tests/_tuner_model.py and
tests/_tuner_formats_model.py extended from Fs_w = R * rf_Fs to rf_Fs = Fs_w * U / D.  Like those files it neither calls nor
links the product's host code, and it is the DEFINITION of the arithmetic: the device bytes have to equal it
(tests/test_gpu_tuner_rational.py).

gcd(U, D) = 1, 1 <= U <= 32, 2 U <= D <= 512.  The prototype low-pass h has T taps (2 .. 4096) and is designed at the rate
U * Fs_w; with Tp = ceil(T / U) it is zero-padded to U * Tp taps.  A call takes n_wide complex samples, n_wide % D == 0, and
yields n_wide * U / D outputs per channel, so every call starts at an output index that is a multiple of U and the outputs
do not depend on how the stream is cut at multiples of D.  For output m of the stream, n_m = floor(m D / U), p_m = m D mod U:

    y_c[m] = Q( e^{-j phi_c(n_m)} * sum_{j<Tp} ( g_c h[p_m + j U] e^{+j phi_c(j)} ) * x[n_m - j] ),                     (*)
    phi_c(n) = 2 pi (w_c n mod 2^32) / 2^32

which is zero-stuffing the mixed capture by U, filtering with h and taking every D-th sample (tuner_rational_f64).  Samples
in front of the stream are zero samples; output 0 has x[0] as its newest sample.  The state is the last Tp - 1 wide
samples and the wide-sample counter.

What changes against _tuner_model.py / _tuner_formats_model.py:
  * w = freq_word(f_c, Fs_w), unchanged.  Tap (p, j) is g h[p + j U] (cos a_j, sin a_j), a_j = 2 pi ((w j mod 2^32) / 2^32):
    the angle depends on j only.
  * ONE s per channel: the largest integer for which every part of every phase is <= 32512 after scaling by 2^s; the same
    range -14 .. 47 (-14 .. 39 for S16).  llround to int16, stored phase-major: re[p * Tp + j], im[p * Tp + j].
  * rejected: 128 * max_p sum_j (|re[p, j]| + |im[p, j]|) > 2^31 - 1 -- the worst case per PHASE, because a phase is what
    one accumulator sums.
  * acc exact in int32 (U8, S8) or in 64 bits (S16); rotation by the same 2^12 table at index
    (w * (n0 + n_m') mod 2^32) >> 20, n0 the counter at the call's start, n_m' = floor(m' D / U) for output m' of the call.
  * out = clamp(128 + ((y + 2^(s+14+B)) >> (s+15+B)), 0, 255); levels (clipped, power) as before.

With U = 1 this is _tuner_model.py's definition with R = D, byte for byte.
"""
from __future__ import annotations

from math import gcd

import numpy as np

import _tuner_formats_model as fm
import _tuner_model as tm

U_MAX, D_MAX = 32, 512


def check_ratio(U, D):
    if not (1 <= U <= U_MAX and 2 * U <= D <= D_MAX and gcd(U, D) == 1):
        raise ValueError(f"ratio {U}/{D}: gcd 1, 1 <= U <= {U_MAX}, 2 U <= D <= {D_MAX}")


def phase_taps(h, U):
    """h float32[T] -> float64[U, Tp]: row p holds h[p + j U], zero past T"""
    h = np.asarray(h, np.float32).astype(np.float64)
    Tp = -(-len(h) // U)
    hp = np.zeros(U * Tp)
    hp[:len(h)] = h
    return hp.reshape(Tp, U).T.copy()


def design_f64(h, U, Fs_w, f_c, gain):
    """-> (w, s, vr, vi): frequency word, scale exponent, the UNROUNDED scaled taps float64[U, Tp]; s None if rejected"""
    hp = phase_taps(h, U)
    w = tm.freq_word(f_c, Fs_w)
    j = np.arange(hp.shape[1], dtype=np.uint64)
    a = 2.0 * np.pi * (((np.uint64(w) * j) % np.uint64(tm.M32)).astype(np.float64) / 4294967296.0)
    g = np.float64(gain) * hp
    gr, gi = g * np.cos(a)[None, :], g * np.sin(a)[None, :]
    m = float(max(np.abs(gr).max(), np.abs(gi).max()))
    if not np.isfinite(m) or m == 0.0:
        return w, None, None, None
    s = int(np.floor(np.log2(tm.LIMIT / m)))
    while np.ldexp(m, s) > tm.LIMIT:
        s -= 1
    while np.ldexp(m, s + 1) <= tm.LIMIT:
        s += 1
    if s < tm.S_MIN or s > tm.S_MAX:
        return w, None, None, None
    return w, s, np.ldexp(gr, s), np.ldexp(gi, s)


def design(h, U, Fs_w, f_c, gain):
    """-> (w, s, re int64[U * Tp], im int64[U * Tp]) phase-major; ValueError for a channel the tuner rejects"""
    if not 1 <= U <= U_MAX:
        raise ValueError("U out of range")
    if not (abs(f_c) < Fs_w / 2) or not np.isfinite(gain):
        raise ValueError("f_c / gain out of range")
    w, s, vr, vi = design_f64(h, U, Fs_w, f_c, gain)
    if s is None:
        raise ValueError("gain x taps rejected")
    re, im = tm.llround(vr), tm.llround(vi)
    if 128 * int((np.abs(re) + np.abs(im)).sum(axis=1).max()) > 2 ** 31 - 1:
        raise ValueError("a phase's accumulator does not fit int32")
    return w, s, re.reshape(-1), im.reshape(-1)


def out_times(M, U, D):
    """outputs 0 .. M-1 of a call -> (n_m' int64[M], p_m' int64[M])"""
    md = np.arange(M, dtype=np.int64) * D
    return md // U, md % U


def accumulate(values, hist, re, im, U, D, fmt):
    """acc of N channels: re, im int64[N, U * Tp] phase-major -> (ar, ai) int64[N, M]; hist: the 2 (Tp - 1) raw values in
    front.  float64 matmuls, one per phase: every partial sum is an integer below 2^53."""
    re, im = np.atleast_2d(re), np.atleast_2d(im)
    N, Tp = re.shape[0], re.shape[1] // U
    assert len(hist) == 2 * (Tp - 1) and len(values) % (2 * D) == 0
    x = np.concatenate([fm.to_x(hist, fmt), fm.to_x(values, fmt)])
    xr, xq = x[0::2].astype(np.float64), x[1::2].astype(np.float64)
    M = len(values) // 2 // D * U
    nm, pm = out_times(M, U, D)
    ar, ai = np.empty((N, M), np.int64), np.empty((N, M), np.int64)
    swr, swq = np.lib.stride_tricks.sliding_window_view(xr, Tp), np.lib.stride_tricks.sliding_window_view(xq, Tp)
    for p in range(U):
        sel = np.nonzero(pm == p)[0]
        fr, fi = re[:, p * Tp:(p + 1) * Tp].T.astype(np.float64), im[:, p * Tp:(p + 1) * Tp].T.astype(np.float64)
        for i in range(0, len(sel), tm.CHUNK):
            mm = sel[i:i + tm.CHUNK]
            wr, wq = swr[nm[mm]][:, ::-1], swq[nm[mm]][:, ::-1]            # [m, j] = x[n_m - j]
            ar[:, mm] = np.rint(wr @ fr - wq @ fi).T.astype(np.int64)
            ai[:, mm] = np.rint(wr @ fi + wq @ fr).T.astype(np.int64)
    lim = 2 ** 40 if fmt == fm.S16 else 2 ** 31
    assert np.abs(ar).max(initial=0) < lim and np.abs(ai).max(initial=0) < lim
    return ar, ai


def rotate_round(ar, ai, w, s, U, D, n0, fmt):
    """one channel -> (out u8[2M], clipped, power): the outputs' newest samples are n0 + floor(m' D / U) (absolute)"""
    sh = s + 15 + fm.EXTRA_BITS[fmt]
    assert 1 <= sh <= 62
    ct, st = tm.table()
    M = len(ar)
    nm, _ = out_times(M, U, D)
    n = (np.uint64(n0 % tm.M32) + nm.astype(np.uint64)) % np.uint64(tm.M32)
    P = (np.uint64(w) * n) % np.uint64(tm.M32)
    i = (P >> np.uint64(32 - tm.TB)).astype(np.int64)
    c, sn = ct[i], st[i]
    yr, yi = ar * c + ai * sn, ai * c - ar * sn
    o = np.empty(2 * M, np.int64)
    o[0::2] = 128 + ((yr + (1 << (sh - 1))) >> sh)
    o[1::2] = 128 + ((yi + (1 << (sh - 1))) >> sh)
    oc = np.clip(o, 0, 255)
    d = oc - 128
    return oc.astype(np.uint8), int(np.count_nonzero(oc != o)), int((d * d).sum())


class TunerRationalModel:
    """The rational tuner as a stream, any format: state = the last Tp - 1 wide samples as raw values and the counter."""

    def __init__(self, h, U, D, n_channels, fmt=fm.U8):
        check_ratio(U, D)
        self.h = np.asarray(h, np.float32)
        self.U, self.D, self.T, self.N, self.fmt = int(U), int(D), len(self.h), int(n_channels), int(fmt)
        assert self.fmt in fm.DTYPES and 2 <= self.T <= 4096
        self.Tp = -(-self.T // self.U)
        self.w = [0] * self.N
        self.s = [0] * self.N
        self.re = np.zeros((self.N, self.U * self.Tp), np.int64)
        self.im = np.zeros((self.N, self.U * self.Tp), np.int64)
        for c in range(self.N):
            self.set_channel(c, 0.0, 1.0, 1.0)
        self.reset()

    def reset(self):
        self.hist = fm.silence(self.Tp, self.fmt)
        self.n = 0
        self.clipped = np.zeros(self.N, np.uint64)
        self.power = np.zeros(self.N, np.uint64)

    def set_channel(self, c, f_c, Fs_w, gain):
        self.set_channel_ints(c, *design(self.h, self.U, Fs_w, f_c, gain))

    def set_channel_ints(self, c, w, s, re, im):
        if not tm.S_MIN <= int(s) <= fm.s_max(self.fmt):
            raise ValueError(f"scale exponent {s} outside {tm.S_MIN} .. {fm.s_max(self.fmt)}")
        self.w[c], self.s[c] = int(w), int(s)
        self.re[c], self.im[c] = np.asarray(re, np.int64), np.asarray(im, np.int64)

    def process(self, values):
        values = fm.raw(values, self.fmt)
        ar, ai = accumulate(values, self.hist, self.re, self.im, self.U, self.D, self.fmt)
        out = np.empty((self.N, 2 * ar.shape[1]), np.uint8)
        for c in range(self.N):
            out[c], cl, pw = rotate_round(ar[c], ai[c], self.w[c], self.s[c], self.U, self.D, self.n, self.fmt)
            self.clipped[c], self.power[c] = cl, pw
        if self.Tp > 1:
            self.hist = np.concatenate([self.hist, values])[-2 * (self.Tp - 1):]
        self.n += len(values) // 2
        return out


# --------------------------------------------------------------------------------------------------------------------
# the float64 statement and the bound
# --------------------------------------------------------------------------------------------------------------------
def tuner_rational_f64(values, hist, h, U, D, cycles_per_sample, gain, fmt, n0=0):
    """The zero-stuffed statement in float64: mix the capture (x in input units) down by cycles_per_sample = f_c / Fs_w,
    put U - 1 zeros between its samples, filter with h, keep every D-th sample, divide by 2^B: complex128[M], the
    unrounded output in LSB.  hist: the 2 (Tp - 1) raw values in front.  The phase is reduced mod 1 cycle before the
    cosine, as in _tuner_model.tuner_f64."""
    h = np.asarray(h, np.float32).astype(np.float64)
    T = len(h)
    Tp = -(-T // U)
    x = np.concatenate([fm.to_x(hist, fmt), fm.to_x(values, fmt)]).astype(np.float64)
    z = x[0::2] + 1j * x[1::2]
    n = np.float64(n0) - (Tp - 1) + np.arange(len(z), dtype=np.float64)
    z = z * np.exp(-2j * np.pi * np.modf(np.float64(cycles_per_sample) * n)[0])
    v = np.zeros(U * len(z) + T, np.complex128)                   # v[U (Tp - 1) + U i] = sample i of the call
    v[T:][0:U * len(z):U] = z                                     # T zeros in front so that every window exists
    M = len(values) // 2 // D * U
    base = T + U * (Tp - 1)                                       # index in v of the call's sample 0
    sw = np.lib.stride_tricks.sliding_window_view(v, T)           # sw[i, t] = v[i + t]
    y = np.empty(M, np.complex128)
    for m in range(0, M, tm.CHUNK):
        mm = np.arange(m, min(m + tm.CHUNK, M))
        y[mm] = sw[base + mm * D - (T - 1)][:, ::-1] @ h            # sum_k h[k] v[base + m D - k]
    return np.float64(gain) * y * 2.0 ** -fm.EXTRA_BITS[fmt]


def tuner_rational_bound(values, hist, re, im, w, s, U, D, cycles_per_sample, fmt, n0=0):
    """Per output sample, the largest distance (in LSB) between the model's byte and clip(128 + tuner_rational_f64).  The
    terms are _tuner_formats_model.tuner_bound's (S = s + B; one output LSB = 2^S units of acc), each re-derived for an
    output that sums ONE phase of the taps over the Tp samples x[n_m - j], j < Tp:

      1/2                                       the final rounding (add half, floor): in output LSB, unchanged
    + sqrt(2) 2^-(S+1) sum_{j<Tp} (|xr| + |xq|)[n_m - j]
                                                tap rounding: output m meets only the Tp taps of its phase p_m, each part
                                                of each off by <= 1/2, so each part of acc by <= 1/2 the sum of |xr| + |xq|
                                                over the Tp samples n_m - Tp + 1 .. n_m that phase meets (a zero-padded
                                                tap rounds exactly, so counting it only loosens the bound); the rotation
                                                turns the error vector, at most sqrt(2) times a part
    + |a| (2 pi / 4096 + 2^-15 (1 + 1/sqrt 2))  a = acc 2^-S: the table index drops up to one table step of phase, the
                                                entries are rounded and scaled 32767 / 32768 -- relative to |a|, unchanged
    + |a| 2 pi |cps - w'/2^32| n                the frequency word's rounding at the output's absolute wide index
                                                n = n0 + n_m: taps and rotation carry the same quantised frequency
    + |a| 2 pi 2^-21 + 1e-9                     float64's own phase error at n up to 2^32, and its summation noise: the
                                                zero-stuffed sum has the same Tp non-zero terms, h there is U times the
                                                integer tuner's and 2^-B x no larger than a byte
    No term comes from the accumulation (exact) or from the resampling: (*) and the zero-stuffed form are the same sum."""
    S = s + fm.EXTRA_BITS[fmt]
    ar, ai = accumulate(values, hist, re, im, U, D, fmt)
    a = np.hypot(ar[0].astype(np.float64), ai[0].astype(np.float64)) * 2.0 ** -S
    Tp = np.atleast_2d(re).shape[1] // U
    u = np.abs(np.concatenate([fm.to_x(hist, fmt), fm.to_x(values, fmt)]).astype(np.float64))
    mag = u[0::2] + u[1::2]
    cs = np.concatenate([[0.0], np.cumsum(mag)])
    nm, _ = out_times(len(a), U, D)
    hi = (Tp - 1) + nm + 1                                        # one past the newest sample (history-extended index)
    sx = cs[hi] - cs[hi - Tp]
    wsig = w - tm.M32 if w >= tm.M32 // 2 else w
    n = np.float64(n0) + nm.astype(np.float64)
    return (0.5 + np.sqrt(2.0) * 2.0 ** -(S + 1) * sx + a * (2 * np.pi / 4096 + 2.0 ** -15 * (1 + np.sqrt(0.5)))
            + a * 2 * np.pi * abs(np.float64(cycles_per_sample) - wsig / 4294967296.0) * n + a * 2 * np.pi * 2.0 ** -21 + 1e-9)
