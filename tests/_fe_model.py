"""Integer model of the matrix-core front end (kernels_fe_mfma.hip), written from its documented arithmetic in plain
numpy.  It does not call or link the product's host code (csrc/fe_mfma_host.hpp): it is the second, independent
statement of what the kernel computes, so that its IF outputs can be checked bit for bit.

The arithmetic:
  * s: the largest integer with max|h| * 2^s <= 127 * 65536 (fe_mfma_scale); tap sets outside it are rejected.
  * q[k] = llround(h[k] * 2^s) (half away from zero), split into three balanced base-256 digits d0, d1, d2 in
    [-128, 127], least significant first: q = d0 + 256 d1 + 65536 d2.
  * x = u8 - 128, exact in int8.  acc_i = sum_k d_i[k] * x[p - k], exact in int32 (the MFMAs).
  * lo = acc0 + 256 acc1 (int32), sc = 2^-(s+7) as float32 (2^-s for the taps, 1/128 for the samples).
  * y = fmaf(float(acc2), 65536 sc, float(lo) * sc): float(lo) rounds once |lo| > 2^24, the product by sc is exact
    unless it is subnormal, and the fma rounds once more.  Two roundings: y is NOT always the correctly rounded
    sum_k q[k] x[p-k] sc, but it is within

        sum_k |x_k|/128 * 2^-(s+1)  +  2^-24 |float(lo) sc|  +  2^-24 |y|   (+ 2^-148 when sc is subnormal)

    of the real-number FIR sum_k h[k] x[p-k] / 128 (fe_bound).

fe_model(iq_u8, hist_u8, h, D) -> (I, Q): output k of a block is the FIR at sample k*D (the newest sample of its
window); samples in front of the block come from the end of hist_u8 (interleaved bytes, like the block).
"""
from __future__ import annotations

import numpy as np

LIMIT = 127.0 * 65536.0        # max |q|: every balanced digit of q fits int8
NDIG = 3
CHUNK = 1 << 15               # outputs per matmul: a chunk's windows are CHUNK * T float64


def fe_scale(h):
    """fe_mfma_scale: s, or None for the tap sets the matrix-core kernel rejects."""
    h = np.asarray(h, np.float32).astype(np.float64)
    if not np.all(np.isfinite(h)):
        return None
    m = float(np.max(np.abs(h)))
    if m == 0.0 or m < 1e-30 or m > 1e30:
        return None
    s = int(np.floor(np.log2(LIMIT / m)))
    while np.ldexp(m, s) > LIMIT:
        s -= 1
    return s


def llround(v):
    """C llround on float64: round half away from zero (np.round rounds half to even)."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def fe_digits(h, s):
    """-> (q int64[T], digits int64[NDIG, T]), digits balanced base 256, least significant first."""
    q = llround(np.ldexp(np.asarray(h, np.float32).astype(np.float64), s))
    r, dig = q.copy(), np.zeros((NDIG, len(q)), np.int64)
    for d in range(NDIG):
        v = ((r + 128) & 255) - 128
        dig[d] = v
        r = (r - v) // 256
    assert not r.any(), "q does not fit NDIG digits"
    return q, dig


def scales(s):
    """(scale_lo, scale_hi) as the kernel has them: float32(2^-(s+7)) and scale_lo * 65536 in float32."""
    lo = np.float32(np.ldexp(1.0, -s - 7))
    return lo, np.float32(lo * np.float32(65536.0))


def windows(iq_u8, hist_u8, T, D, channel, k0=0):
    """Yields (k_start, W) with W[j, t] = x[p_j - t] (float64, x = u8 - 128) of channel 0 (I) / 1 (Q) for the outputs
    k = k_start + j, p_j = k*D, in chunks.  Outputs from k0 (negative k: in front of the block) to n // D - 1."""
    iq = np.asarray(iq_u8, np.uint8)
    hist = np.asarray(hist_u8, np.uint8)
    assert len(iq) % 2 == 0 and len(hist) % 2 == 0
    n, nh = len(iq) // 2, len(hist) // 2
    xs = np.concatenate([hist[channel::2], iq[channel::2]]).astype(np.int16) - 128
    n_out = n // D
    assert nh + k0 * D - (T - 1) >= 0, "history too short"
    sw = np.lib.stride_tricks.sliding_window_view(xs, T)   # sw[i, t] = xs[i + t]: newest sample at t = T-1
    for k in range(k0, n_out, CHUNK):
        kk = np.arange(k, min(k + CHUNK, n_out))
        w = sw[nh + kk * D - (T - 1)][:, ::-1]
        yield k, w.astype(np.float64)


def epilogue(acc, s):
    """acc int64[NDIG, n] -> float32[n] as the kernel's epilogue computes it; also returns float(lo)*sc as float64."""
    lo = acc[0] + 256 * acc[1]
    assert np.all(np.abs(lo) < 2 ** 31), "lo overflows int32"
    assert np.all(np.abs(acc[2]) < 2 ** 31), "acc2 overflows int32"
    sc_lo, sc_hi = scales(s)
    flo = (lo.astype(np.float32) * sc_lo).astype(np.float64)             # two float32 roundings, as the kernel's
    hi = acc[2].astype(np.float32).astype(np.float64) * np.float64(sc_hi)   # exact: a float32 times a power of two
    return round_sum_f32(hi, flo), flo


def round_sum_f32(a, b):
    """float32(a + b) rounded ONCE (what fmaf does with an exact product): the float64 sum is exact unless the float32
    operands span more than 53 bits (subnormal flo); then it is RN53 of the exact sum, which is rounded again correctly
    unless it lands on a float32 midpoint, where the sign of the TwoSum residual decides."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)                                  # TwoSum: s + err == a + b exactly
    f = s.astype(np.float32)
    fix = err != 0
    if fix.any():
        sf, ff, ef = s[fix], f[fix], err[fix]
        other = np.nextafter(ff, np.where(sf > ff.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)))
        mid = (ff.astype(np.float64) + other.astype(np.float64)) / 2
        tie = sf == mid
        up = np.where(ef > 0, np.maximum(ff, other), np.minimum(ff, other))
        f[np.flatnonzero(fix)[tie]] = up[tie]
    return f


def fe_channel_acc(iq_u8, hist_u8, h, D, channel, k0=0):
    """The three exact digit accumulators of one channel's outputs k0 .. n//D - 1 (int64[NDIG, n_out - k0])."""
    s = fe_scale(h)
    assert s is not None, "taps the matrix-core kernel rejects"
    _, dig = fe_digits(h, s)
    T = len(h)
    parts = [np.rint(w @ dig.T.astype(np.float64)).astype(np.int64).T     # exact: every |acc| < 2^53
             for _, w in windows(iq_u8, hist_u8, T, D, channel, k0)]
    return np.concatenate(parts, axis=1) if parts else np.zeros((NDIG, 0), np.int64)


def fe_model(iq_u8, hist_u8, h, D, k0=0):
    """IF (I, Q) float32 of one block, bit for bit as the matrix-core kernel computes it."""
    s = fe_scale(h)
    return tuple(epilogue(fe_channel_acc(iq_u8, hist_u8, h, D, c, k0), s)[0] for c in (0, 1))


def fe_f64(iq_u8, hist_u8, h, D, k0=0):
    """The real FIR sum_k h[k] x[p-k] / 128 in float64 -> (I, Q, sum_k |x_k| per output of I, ... of Q)."""
    h64 = np.asarray(h, np.float32).astype(np.float64)
    out = []
    for c in (0, 1):
        ys, ax = [], []
        for _, w in windows(iq_u8, hist_u8, len(h), D, c, k0):
            ys.append(w @ h64 / 128.0)
            ax.append(np.abs(w).sum(axis=1))
        out.append((np.concatenate(ys) if ys else np.zeros(0), np.concatenate(ax) if ax else np.zeros(0)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def fe_bound(y, flo, sum_abs_x, s):
    """|y - fe_f64| <= this (see the module docstring): tap quantisation, float(lo), the fma's rounding."""
    sc_lo, _ = scales(s)
    b = sum_abs_x / 128.0 * np.ldexp(1.0, -(s + 1)) + 2.0 ** -24 * np.abs(flo) + 2.0 ** -24 * np.abs(np.asarray(y, np.float64))
    if sc_lo < np.finfo(np.float32).tiny:
        b = b + 2.0 ** -148
    return b


def fe_check(iq_u8, hist_u8, h, D, got_i, got_q, k0=0, msg=""):
    """Asserts got_i / got_q are bit-equal to fe_model and, independently, that the model is within fe_bound of the
    float64 FIR.  One pass over the windows per channel.  Returns the model's (I, Q)."""
    s = fe_scale(h)
    assert s is not None, "taps the matrix-core kernel rejects"
    _, dig = fe_digits(h, s)
    m = np.concatenate([dig.T.astype(np.float64), np.asarray(h, np.float32).astype(np.float64)[:, None]], axis=1)
    out = []
    for c, got in enumerate((got_i, got_q)):
        acc, f64, ax = [], [], []
        for _, w in windows(iq_u8, hist_u8, len(h), D, c, k0):
            r = w @ m
            acc.append(np.rint(r[:, :NDIG]).astype(np.int64).T)           # exact: every |acc| < 2^53
            f64.append(r[:, NDIG] / 128.0)
            ax.append(np.abs(w).sum(axis=1))
        acc = np.concatenate(acc, axis=1) if acc else np.zeros((NDIG, 0), np.int64)
        f64 = np.concatenate(f64) if f64 else np.zeros(0)
        ax = np.concatenate(ax) if ax else np.zeros(0)
        want, flo = epilogue(acc, s)
        got = np.asarray(got, np.float32)
        assert got.shape == want.shape, (msg, "IQ"[c], got.shape, want.shape)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f"{msg} {'IQ'[c]}: {bad.size} of {got.size} outputs differ from the integer model, first at "
                               f"{bad[:8].tolist()}: got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}")
        err = np.abs(want.astype(np.float64) - f64)
        bnd = fe_bound(want, flo, ax, s)
        assert np.all(err <= bnd), (msg, "IQ"[c], "model outside the float64 bound", float(np.max(err - bnd)))
        out.append(want)
    return tuple(out)


def discriminator_f64(i, q, pi, pq):
    """fmDemod (src/filter.cpp:248-266) in float64 on float32 operands: (i (q - pq) - q (i - pi)) / (i^2 + q^2), 0 where
    the denominator is 0.  Also returns the float64 |i||q - pq| + |q||i - pi| and den for error bounds."""
    i, q, pi, pq = (np.asarray(v, np.float32).astype(np.float64) for v in (i, q, pi, pq))
    a, b = i * (q - pq), q * (i - pi)
    den = i * i + q * q
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(den == 0, 0.0, (a - b) / np.where(den == 0, 1.0, den))
    return d, np.abs(a) + np.abs(b), den
