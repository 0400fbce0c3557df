"""The de-emphasis filter's definition: what every device path computes, bit for bit.

Coefficients (float64 on the host, then rounded to float32): the bilinear transform of 1 / (1 + s tau), pre-warped at the corner:

    k = -tan(1 / (2 fs tau)),  p = (1 + k) / (1 - k),  b0 = (1 - p) / 2

Recurrence per row, state (x_prev, y_prev) = (+0, +0) at the start of a stream:

    u = x[n] + x_prev            one float32 add
    v = b0 * u                   one float32 multiply
    y = fmaf(p, y_prev, v)       one fused multiply-add
    if |y| < 2**-126: y = +0     explicit flush, whatever the hardware's denormal mode

`serial` walks that; `parallel` is the device's scheme -- lanes that own a segment of L samples, start W samples early with
y = +0 (or at sample 0 from the carried state), a verify step that compares each segment's start y with its predecessor's true
end, and a serial repair of the misses -- and returns the same bits, plus the number of misses.  Two values are "the same" when
their bits are equal or both are NaN: NaN payloads are not part of the definition.

Arrays are [rows, n] float32; everything is vectorised over the rows (and the lanes), the time axis is walked in Python."""
import math

import numpy as np

import _walk_events as we
from _fir_model import fmaf
from _walk_events import same  # noqa: F401

F32 = np.float32
FLT_MIN = F32(2.0 ** -126)
BUILTIN_W, BUILTIN_L = 256, 256   # kDeemphWarmup, kDeemphSegment (fmrx_internal.hpp)


def design(fs, tau_us):
    """(p, b0) as float32, or None where fmrx_deemph_design returns FMRX_EINVAL."""
    if not (fs > 0 and tau_us > 0):
        return None
    tau = tau_us * 1e-6
    a = 1.0 / (2.0 * fs * tau)
    if not a < math.pi / 4:
        return None
    k = -math.tan(a)
    p = (1.0 + k) / (1.0 - k)
    b0 = (1.0 - p) / 2.0
    return F32(p), F32(b0)


def step(x, x_prev, y_prev, p, b0):
    """One step of the recurrence on float32 arrays of one shape."""
    with np.errstate(all="ignore"):
        u = (x + x_prev).astype(F32)
        v = (F32(b0) * u).astype(F32)
        y = fmaf(np.full(np.shape(v), p, F32), y_prev, v)
        return np.where(np.abs(y) < FLT_MIN, F32(0.0), y).astype(F32)


def _rows(x, state):
    x = np.atleast_2d(np.asarray(x, F32))
    st = np.zeros((x.shape[0], 2), F32) if state is None else np.array(state, F32).reshape(x.shape[0], 2)
    return x, st


def serial(x, p, b0, state=None):
    """-> (y [rows, n], state [rows, 2])."""
    x, st = _rows(x, state)
    y = np.zeros_like(x)
    xp, yp = st[:, 0].copy(), st[:, 1].copy()
    for i in range(x.shape[1]):
        yp = step(x[:, i], xp, yp, p, b0)
        xp = x[:, i]
        y[:, i] = yp
    return y, np.stack([xp, yp], axis=1).astype(F32)


def parallel(x, p, b0, state=None, W=BUILTIN_W, L=BUILTIN_L):
    """The speculate / verify / repair walk -> (y [rows, n], state [rows, 2], missed, checked segments)."""
    y, st, missed, segs = parallel_rows(x, p, b0, state, W, L)
    return y, st, int(missed.sum()), segs


def speculate(x, p, b0, state=None, W=BUILTIN_W, L=BUILTIN_L):
    """The lanes' half of the walk (_walk_events.lanes with this filter's step) -> (y [rows, n], start, end [rows, nseg])."""
    x, st = _rows(x, state)
    xpad = np.concatenate([st[:, :1], x], axis=1)           # xpad[:, g] = x[g - 1]; the carried x_prev in front
    return we.lanes(lambda r, g, yp: step(x[r, g], xpad[r, g], yp, p, b0), st[:, 1], x.shape[1], W, L)


def row_step(x, x_prev, p, b0):
    """One row's step for _walk_events.verify: (g, y) -> y on Python floats.  v = b0 (x[g] + x[g-1]) does not depend on y."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        v = (F32(b0) * (x + np.concatenate([[F32(x_prev)], x[:-1]])).astype(F32)).astype(F32).astype(np.float64).tolist()
    pf, tiny = float(p), float(FLT_MIN)

    def one(g, y):
        r = we.fmaf1(pf, y, v[g])
        return 0.0 if abs(r) < tiny else r
    return one


def parallel_rows(x, p, b0, state=None, W=BUILTIN_W, L=BUILTIN_L, spec=None):
    """parallel() with the misses per row (rows are independent: the first r rows of a result are the result of the first r rows).
    spec: what speculate() returned for these arguments, where the caller has it already."""
    x, st = _rows(x, state)
    rows, n = x.shape
    if n == 0:
        return x.copy(), st, np.zeros(rows, np.int64), 0
    nseg = (n + L - 1) // L
    xpad = np.concatenate([st[:, :1], x], axis=1)
    y, start, end = (v.copy() for v in (spec if spec is not None else speculate(x, p, b0, st, W, L)))
    # ---- verify, in order, and repair: vectorised over the rows that miss ----
    missed = np.zeros(rows, np.int64)
    for c in range(1, nseg):
        miss = np.flatnonzero(~same(start[:, c], end[:, c - 1]))
        missed[miss] += 1
        if len(miss) == 0:
            continue
        yv = end[miss, c - 1].copy()
        live = np.ones(len(miss), bool)                      # rows whose recomputed y has not met the stored one yet
        for g in range(c * L, min(n, (c + 1) * L)):
            yv = step(x[miss, g], xpad[miss, g], yv, p, b0)
            live &= ~same(yv, y[miss, g])
            if not live.any():
                break
            y[miss[live], g] = yv[live]
        end[miss[live], c] = yv[live]
    state_out = np.stack([x[:, -1], end[:, -1]], axis=1).astype(F32)
    return y, state_out, missed, rows * (nseg - 1)


def fixed_inputs(n=4096, fs=48000.0):
    """The three fixed rows of the tests: `audio`, `audio->silence`, `impulse`."""
    rng = np.random.default_rng(7)
    t = np.arange(n) / fs
    audio = (0.4 * np.sin(2 * np.pi * 1e3 * t) + 0.2 * np.sin(2 * np.pi * 7e3 * t) + 0.05 * rng.standard_normal(n)).astype(F32)
    silence = audio.copy()
    silence[1500:] = 0
    impulse = (1e-3 * rng.standard_normal(n)).astype(F32)
    impulse[700] = F32(1e30)
    return {"audio": audio, "audio->silence": silence, "impulse": impulse}
