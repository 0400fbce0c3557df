"""The variable high-cut stage's definition (include/fmrx.h: fmrx_highcut_*), plain numpy, no GPU.
The host function (fmrx_highcut_control) and the kernels equal this file bit for bit.

Design, float64 on the host: p_max_d = exp(-2 pi fc_min / audio_Fs), p_max = float32(p_max_d); refused unless everything is
finite, fc_min > 0, audio_Fs > 0 and p_max <= 0.875.  The pole moves linearly with the cut from 0 (transparent) to p_max.

Control, float64, per channel and call, from the MPX group of the channel's meter record; every step one IEEE operation in
the order written, the blend's helpers (_blend_model: drive, plog2, ramp, smooth) as they are:

    noise = (probe[17k] + probe[21k]) * 0.5;   d_q = drive(ref1 * segments, noise)          as blend's control step forms them
    t_o = (1 - cut_max) + cut_max * ramp(d_q; hc_lo, hc_hi)                                  openness: 1 = no cut
    first call after create / reset: s_o = t_o; else smooth(s_o, t_o): attack where t_o < s_o, release otherwise, the 2^-10 snap
    p1 = float32((1 - s_o) * p_max_d);   p0 = the previous call's p1 (a first call: this call's)

Apply, float32, per row (both rows of a stereo channel use the channel's poles), y_prev = +0 at the start of a stream and
carried across calls; sample k of the call's n, inv_n = float32(1.0 / n):

    p[k] = clamp(fmaf(float32(k + 1), (p1 - p0) * inv_n, p0), 0, p_max)
    q = 1 - p[k];  v = q * x[k];  y = fmaf(p[k], y_prev, v);  if |y| < 2**-126: y = +0
    y[k] = x[k] where p[k] == 0 else y;   y_prev = y[k]

`serial` walks that; `parallel` is the device's scheme (DESIGN.md 4.10 with a pole that moves): lanes that own a segment of L
samples start W samples early from y = +0 (or at sample 0 from the carried state), a verify step compares each segment's
start y with its predecessor's true end on bits (two NaNs count as equal), misses are walked again serially.  It returns
serial's bits plus the number of misses, for any (W, L).

Arrays are [rows, n] float32, the poles one (p0, p1) per row; the time axis is walked in Python."""
from __future__ import annotations

import math

import numpy as np

import _blend_model as bm
from _blend_model import DB_PER_OCTAVE, P_NOISE_HI, P_NOISE_LO, drive, interleave, ramp, smooth  # noqa: F401
from _deemph_model import FLT_MIN, fixed_inputs, same  # noqa: F401
import _walk_events as we
from _fir_model import fmaf

F32, F64 = np.float32, np.float64
P_MAX_CAP = F32(0.875)
BUILTIN_W, BUILTIN_L = 256, 256   # kHighcutWarmup, kHighcutSegment (fmrx_internal.hpp)

DEFAULTS = dict(fc_min=2500.0, hc_lo=16.0, hc_hi=36.0, cut_max=1.0, attack=1.0, release=0.25, warmup=-1, segment=-1)
PARAM_NAMES = tuple(DEFAULTS)
STATUS_DTYPE = np.dtype([("quiet_db", "<f8"), ("open_target", "<f8"), ("open", "<f8"), ("p0", "<f4"), ("p1", "<f4"), ("calls", "<u8")])
assert STATUS_DTYPE.itemsize == 40


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def design(fc_min: float, audio_Fs: float):
    """(p_max_d, p_max), or None where the library returns FMRX_EINVAL."""
    if not (math.isfinite(fc_min) and math.isfinite(audio_Fs) and fc_min > 0.0 and audio_Fs > 0.0):
        return None
    p_max_d = math.exp(((-2.0 * 3.14159265358979323846) * fc_min) / audio_Fs)
    p_max = F32(p_max_d)
    if not p_max <= P_MAX_CAP:
        return None
    return p_max_d, p_max


def valid(p: dict, if_Fs: float, audio_Fs: float) -> bool:
    v = [float(p[k]) for k in PARAM_NAMES[:6]]
    if not all(math.isfinite(x) for x in v) or not (math.isfinite(if_Fs) and if_Fs > 0):
        return False
    if design(p["fc_min"], audio_Fs) is None:
        return False
    if not (p["hc_hi"] > p["hc_lo"] and 0.0 <= p["cut_max"] <= 1.0 and 0.0 < p["attack"] <= 1.0 and 0.0 < p["release"] <= 1.0):
        return False
    return -1 <= int(p["warmup"]) <= 1 << 20 and int(p["segment"]) in range(-1, (1 << 20) + 1) and int(p["segment"]) != 0


def shape(p: dict):
    """(W, L) of the lanes"""
    return (BUILTIN_W if p["warmup"] < 0 else int(p["warmup"])), (BUILTIN_L if p["segment"] < 0 else int(p["segment"]))


def control(p: dict, if_Fs: float, audio_Fs: float) -> dict:
    """The parameters as the step uses them (highcut::Control)."""
    assert valid(p, if_Fs, audio_Fs)
    p_max_d, p_max = design(p["fc_min"], audio_Fs)
    c = dict(hc_lo=p["hc_lo"] / DB_PER_OCTAVE, cut_max=float(p["cut_max"]), floor=1.0 - p["cut_max"], attack=float(p["attack"]),
             release=float(p["release"]), p_max_d=p_max_d, p_max=p_max)
    c["hc_inv"] = 1.0 / (p["hc_hi"] / DB_PER_OCTAVE - c["hc_lo"])
    w = ((2.0 * 3.14159265358979323846 * 7500.0) / float(if_Fs)) * 256.0
    c["ref1"] = w * w
    return c


def fresh(n=None) -> np.ndarray:
    return np.zeros(() if n is None else n, STATUS_DTYPE)


def step(c: dict, rec, st) -> np.ndarray:
    """One channel's control step: c from control(), rec a meter record (probe, segments), st a STATUS_DTYPE scalar -> the new one."""
    with np.errstate(all="ignore"):
        probe = [float(v) for v in rec["probe"]]
        noise = float((F64(probe[P_NOISE_LO]) + F64(probe[P_NOISE_HI])) * F64(0.5))
        dq = drive(float(F64(c["ref1"]) * F64(float(int(rec["segments"])))), noise)
        first = int(st["calls"]) == 0
        t = c["floor"] + c["cut_max"] * ramp(dq, c["hc_lo"], c["hc_inv"])
        s = smooth(float(st["open"]), t, first, c)
        p1 = F32((1.0 - s) * c["p_max_d"])
        out = np.zeros((), STATUS_DTYPE)
        out["p0"] = p1 if first else st["p1"]
        out["p1"] = p1
        out["quiet_db"] = F64(dq) * F64(DB_PER_OCTAVE)
        out["open_target"], out["open"] = t, s
        out["calls"] = int(st["calls"]) + 1
    return out


def step_all(c: dict, recs, state) -> np.ndarray:
    return np.array([step(c, recs[i], state[i]) for i in range(len(recs))], STATUS_DTYPE)


# ---- apply ----------------------------------------------------------------------------------------------------------
def poles(p0, p1, n, p_max) -> np.ndarray:
    """[rows, n] float32: p[k] of each row."""
    p0, p1 = np.atleast_1d(np.asarray(p0, F32)), np.atleast_1d(np.asarray(p1, F32))
    inv_n = F32(1.0 / n)
    st = ((p1 - p0).astype(F32) * inv_n).astype(F32)
    k1 = (np.arange(n, dtype=np.int64) + 1).astype(F32)
    x = fmaf(k1[None, :], st[:, None], p0[:, None])
    return np.where(x < 0, F32(0), np.where(x > F32(p_max), F32(p_max), x)).astype(F32)


def filt(x, p, y_prev):
    """One step on float32 arrays of one shape."""
    with np.errstate(all="ignore"):
        q = (F32(1.0) - p).astype(F32)
        v = (q * x).astype(F32)
        y = fmaf(p, y_prev, v)
        y = np.where(np.abs(y) < FLT_MIN, F32(0.0), y).astype(F32)
        return np.where(p == 0, x, y).astype(F32)


def _rows(x, p0, p1, state):
    x = np.atleast_2d(np.asarray(x, F32))
    rows = x.shape[0]
    st = np.zeros(rows, F32) if state is None else np.array(state, F32).reshape(rows)
    return x, np.broadcast_to(np.asarray(p0, F32), (rows,)), np.broadcast_to(np.asarray(p1, F32), (rows,)), st


def serial(x, p0, p1, p_max, state=None):
    """-> (y [rows, n], state [rows])."""
    x, p0, p1, yp = _rows(x, p0, p1, state)
    y = np.zeros_like(x)
    if x.shape[1] == 0:
        return y, yp
    P = poles(p0, p1, x.shape[1], p_max)
    yp = yp.copy()
    for i in range(x.shape[1]):
        yp = filt(x[:, i], P[:, i], yp)
        y[:, i] = yp
    return y, yp


def parallel(x, p0, p1, p_max, state=None, W=BUILTIN_W, L=BUILTIN_L):
    """The speculate / verify / repair walk -> (y [rows, n], state [rows], missed, checked segments)."""
    y, st, missed, segs = parallel_rows(x, p0, p1, p_max, state, W, L)
    return y, st, int(missed.sum()), segs


def speculate(x, p0, p1, p_max, state=None, W=BUILTIN_W, L=BUILTIN_L):
    """The lanes' half of the walk (_walk_events.lanes with this filter's step) -> (y [rows, n], start, end [rows, nseg])."""
    x, p0, p1, st = _rows(x, p0, p1, state)
    P = poles(p0, p1, x.shape[1], p_max)
    return we.lanes(lambda r, g, yp: filt(x[r, g], P[r, g], yp), st, x.shape[1], W, L)


def row_step(x, p0, p1, p_max):
    """One row's step for _walk_events.verify: (g, y) -> y on Python floats.  p[g], q and v = q x[g] do not depend on y."""
    x = np.asarray(x, F32)
    P = poles(p0, p1, len(x), p_max)[0]
    with np.errstate(all="ignore"):
        v = ((F32(1.0) - P).astype(F32) * x).astype(F32).astype(F64).tolist()
    xs, Ps, tiny = x.astype(F64).tolist(), P.astype(F64).tolist(), float(FLT_MIN)

    def one(g, y):
        if Ps[g] == 0.0:
            return xs[g]
        r = we.fmaf1(Ps[g], y, v[g])
        return 0.0 if abs(r) < tiny else r
    return one


def parallel_rows(x, p0, p1, p_max, state=None, W=BUILTIN_W, L=BUILTIN_L, spec=None):
    """parallel() with the misses per row.  spec: what speculate() returned for these arguments, where the caller has it."""
    x, p0, p1, st = _rows(x, p0, p1, state)
    rows, n = x.shape
    if n == 0:
        return x.copy(), st, np.zeros(rows, np.int64), 0
    P = poles(p0, p1, n, p_max)
    nseg = (n + L - 1) // L
    y, start, end = (v.copy() for v in (spec if spec is not None else speculate(x, p0, p1, p_max, st, W, L)))
    missed = np.zeros(rows, np.int64)
    for c in range(1, nseg):
        miss = np.flatnonzero(~same(start[:, c], end[:, c - 1]))
        missed[miss] += 1
        if len(miss) == 0:
            continue
        yv = end[miss, c - 1].copy()
        live = np.ones(len(miss), bool)                      # rows whose recomputed y has not met the stored one yet
        for g in range(c * L, min(n, (c + 1) * L)):
            yv = filt(x[miss, g], P[miss, g], yv)
            live &= ~same(yv, y[miss, g])
            if not live.any():
                break
            y[miss[live], g] = yv[live]
        end[miss[live], c] = yv[live]
    return y, end[:, -1].astype(F32).copy(), missed, rows * (nseg - 1)


def apply(c, status, audio, state=None, W=None, L=None):
    """c from control(); status: STATUS_DTYPE [N] after the call's control step; audio [N, ac, n]; state [N * ac] or None ->
    (y of the same shape, state [N * ac], missed, checked segments): the serial walk where W is None, else the parallel one."""
    a = np.asarray(audio, F32)
    N, ac, n = a.shape
    p0, p1 = np.repeat(status["p0"], ac), np.repeat(status["p1"], ac)
    if W is None:
        y, st = serial(a.reshape(N * ac, n), p0, p1, c["p_max"], state)
        return y.reshape(a.shape), st, 0, 0
    y, st, missed, segs = parallel(a.reshape(N * ac, n), p0, p1, c["p_max"], state, W, L)
    return y.reshape(a.shape), st, missed, segs


def response(p, f, fs):
    """|(1 - p) / (1 - p e^{-j w})| in float64"""
    w = 2.0 * math.pi * f / fs
    return abs((1.0 - p) / (1.0 - p * np.exp(-1j * w)))


# ---- what the tests feed ---------------------------------------------------------------------------------------------
rec, rec_for, hand_made_records, random_rows = bm.rec, bm.rec_for, bm.hand_made_records, bm.random_rows

PARAM_SETS = {"defaults": {}, "half and slow": dict(cut_max=0.5, attack=0.5, release=0.125, fc_min=4000.0),
              "narrow": dict(hc_lo=-3.0, hc_hi=40.0, fc_min=1100.0)}


def sequences(c):
    """name -> list of records, or None = reset before the next one.  Quieting drives in dB."""
    def r(quiet_db):
        return rec_for(c, 40.0 / DB_PER_OCTAVE, quiet_db / DB_PER_OCTAVE)
    return {
        "walk": [r(40), r(26), r(10), r(26), r(40), r(40)],            # cut 0 -> partial -> full -> partial -> 0
        "attack and release": [r(40), r(17)] + [r(40)] * 26,
        "partial": [r(20), r(30), r(24), r(33)],
        "reset": [r(40), r(5), None, r(40), r(26), None, r(5), r(40)],
        "full": [r(5)] * 3 + [r(40)] * 3,
    }
