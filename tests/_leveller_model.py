"""The loudness leveller and look-ahead peak limiter's definition (include/fmrx.h: fmrx_leveller_*),
plain numpy, no GPU.  The host functions (fmrx_leveller_control, fmrx_leveller_walk) and both kernels equal this file bit for
bit.

Control, float64, per channel and call, from the audio meters' record (n, sum_k2).  Every step is one IEEE operation, in the
order written; no fused multiply-add, no sqrt, no log.  The dB parameters become linear values once, with libm's pow
(math.pow here, the same function):

    fs2 = full_scale * full_scale
    target_ms = pow(10, (target_lkfs + 0.691) / 10)      gate_ms = pow(10, (gate_lkfs + 0.691) / 10)
    g_max = pow(10, max_boost_db / 20)                    g_min = pow(10, -max_cut_db / 20)
    c = float32(full_scale * pow(10, ceiling_dbfs / 20))  the limiter's ceiling

    ms = ((sum_k2[0] + (sum_k2[1] if stereo else 0)) / float64(n)) / fs2
    gated = not (ms >= gate_ms and ms < inf)       NaN, n = 0 and an infinite sum included: loud_ms stands
    otherwise: loud_ms = ms where there is no estimate yet (loud_ms is not > 0), else loud_ms + k * (ms - loud_ms),
               k = attack where ms > loud_ms else release
    gain = 1 where there is no estimate; else r = target_ms / loud_ms: g_min where r is not > 0, g_max where r is infinite,
           else heron2(r) clamped to [g_min, g_max]
    heron2(r): x = 0.5 * plog2(r) (the blend's Mitchell pseudo-logarithm); f = floor(x); y = ldexp(1 + (x - f), f);
               twice y = 0.5 * (y + r / y)
    gain1 = float32(gain); gain0 = the previous call's gain1 (a first call: this call's); min_code = 2^24, limited = 0

Gain and limiter, float32 and integers, per channel; W the look-ahead (a power of two, 8 .. 128), ONE = 2^24, sample k of the
call's n, inv_n = float32(1.0 / n):

    g[k] = fmaf(float32(k + 1), (gain1 - gain0) * inv_n, gain0)
    u_r[k] = x_r[k] * g[k]
    code(a) = ONE where a <= c; else uint32((c / a) * 16777216.0f) (truncated) where a < inf; else 0 (NaN and infinity)
    q[k] = min over the rows of code(|u_r[k]|)
    m[k] = min(q[k-W+1 .. k]);   s[k] = (sum of m[k-W+1 .. k]) >> log2 W
    y_r[k] = u_r[k-(W-1)] * (float32(s[k]) * 2^-24)
    min_code = min s[k], limited = the number of k with s[k] < ONE, over the call

The state per channel: the last 2W-2 codes and the last W-1 values of u per row; fresh: ONE and zeros.

Two floats are "the same" when their bits are equal or both are NaN (_deemph_model.same)."""
from __future__ import annotations

import math

import numpy as np

from _blend_model import plog2
from _deemph_model import same  # noqa: F401  (the tests' comparison)
from _fir_model import fmaf

F32, F64 = np.float32, np.float64
ONE = 1 << 24
LOOKAHEADS = (8, 16, 32, 64, 128)

DEFAULTS = dict(target_lkfs=-23.0, max_boost_db=12.0, max_cut_db=20.0, gate_lkfs=-50.0, attack=0.2, release=0.02, ceiling_dbfs=-1.0,
                full_scale=2.0)
PARAM_NAMES = tuple(DEFAULTS)
STATUS_DTYPE = np.dtype([("loud_ms", "<f8"), ("gain", "<f8"), ("gain0", "<f4"), ("gain1", "<f4"), ("gated", "<u4"), ("min_code", "<u4"),
                         ("limited", "<u4"), ("reserved", "<u4"), ("calls", "<u8")])
assert STATUS_DTYPE.itemsize == 48
# the part of tests/test_audio_meters_model_host's record the control step reads
AUDIO_METER_DTYPE = np.dtype([("n", "<u8"), ("over", "<u8", (2,)), ("peak", "<f8", (2,)), ("sum_x", "<f8", (2,)), ("sum_x2", "<f8", (2,)),
                              ("sum_k2", "<f8", (2,)), ("sum_lr", "<f8"), ("bins_done", "<u8")])
assert AUDIO_METER_DTYPE.itemsize == 104


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _linear(p: dict) -> dict:
    fs = float(p["full_scale"])
    with np.errstate(all="ignore"):
        try:
            return dict(fs2=fs * fs, target_ms=math.pow(10.0, (p["target_lkfs"] + 0.691) / 10.0),
                        gate_ms=math.pow(10.0, (p["gate_lkfs"] + 0.691) / 10.0), g_max=math.pow(10.0, p["max_boost_db"] / 20.0),
                        g_min=math.pow(10.0, -p["max_cut_db"] / 20.0), attack=float(p["attack"]), release=float(p["release"]),
                        ceiling=F32(fs * math.pow(10.0, p["ceiling_dbfs"] / 20.0)))
        except OverflowError:
            return dict(fs2=math.inf)


def valid(p: dict) -> bool:
    v = [float(p[k]) for k in PARAM_NAMES]
    if not all(math.isfinite(x) for x in v):
        return False
    if not (p["max_boost_db"] >= 0.0 and p["max_cut_db"] >= 0.0 and p["gate_lkfs"] < p["target_lkfs"] and 0.0 < p["attack"] <= 1.0
            and 0.0 < p["release"] <= 1.0 and p["ceiling_dbfs"] < 0.0 and p["full_scale"] > 0.0):
        return False
    c = _linear(p)
    if len(c) == 1:
        return False
    return (all(math.isfinite(c[k]) and c[k] > 0.0 for k in ("fs2", "target_ms", "gate_ms", "g_max", "g_min"))
            and bool(np.isfinite(c["ceiling"])) and float(c["ceiling"]) >= 2.0 ** -126)


def control(p: dict) -> dict:
    """The parameters as the step uses them (leveller::Control)."""
    assert valid(p)
    return _linear(p)


def pexp2(x: float) -> float:
    f = math.floor(x)
    return math.ldexp(1.0 + (x - f), int(f))


def heron2(r: float) -> float:
    """The square root of a finite r > 0 in basic operations."""
    y = pexp2(0.5 * plog2(r))
    with np.errstate(all="ignore"):
        y = float(F64(0.5) * (F64(y) + F64(r) / F64(y)))
        y = float(F64(0.5) * (F64(y) + F64(r) / F64(y)))
    return y


def fresh(n=None) -> np.ndarray:
    return np.zeros(() if n is None else n, STATUS_DTYPE)


def rec(n=1920, k2=(0.0, 0.0)) -> np.ndarray:
    r = np.zeros((), AUDIO_METER_DTYPE)
    r["n"] = n
    r["sum_k2"] = k2
    return r


def rec_for(c: dict, lkfs: float, n=1920, ac=2) -> np.ndarray:
    """A record that reads about `lkfs` LKFS, the energy split over the rows 3 : 1."""
    total = math.pow(10.0, (lkfs + 0.691) / 10.0) * c["fs2"] * n
    return rec(n, (0.75 * total, 0.25 * total) if ac == 2 else (total, 0.0))


def step(c: dict, ac: int, record, st) -> np.ndarray:
    """One channel's control step: c from control(), record an audio meter record (n, sum_k2), st a STATUS_DTYPE scalar -> the
    new one."""
    with np.errstate(all="ignore"):
        k2 = F64(record["sum_k2"][0]) + (F64(record["sum_k2"][1]) if ac == 2 else F64(0.0))
        ms = float((k2 / F64(float(int(record["n"])))) / F64(c["fs2"]))
        gated = not (ms >= c["gate_ms"] and ms < math.inf)
        loud = float(st["loud_ms"])
        if not gated:
            if not loud > 0.0:
                loud = ms
            else:
                k = c["attack"] if ms > loud else c["release"]
                loud = float(F64(loud) + F64(k) * (F64(ms) - F64(loud)))
        gain = 1.0
        if loud > 0.0:
            r = float(F64(c["target_ms"]) / F64(loud))
            if not r > 0.0:
                gain = c["g_min"]
            elif math.isinf(r):
                gain = c["g_max"]
            else:
                y = heron2(r)
                gain = c["g_min"] if y < c["g_min"] else (c["g_max"] if y > c["g_max"] else y)
        first = int(st["calls"]) == 0
        out = np.zeros((), STATUS_DTYPE)
        gain1 = F32(gain)
        out["loud_ms"], out["gain"], out["gain1"], out["gain0"] = loud, gain, gain1, gain1 if first else st["gain1"]
        out["gated"], out["min_code"], out["limited"], out["calls"] = int(gated), ONE, 0, int(st["calls"]) + 1
    return out


def step_all(c: dict, ac: int, recs, state) -> np.ndarray:
    return np.array([step(c, ac, recs[i], state[i]) for i in range(len(recs))], STATUS_DTYPE)


# ---- the gain and the limiter --------------------------------------------------------------------------------------------
def fresh_state(ac: int, W: int) -> dict:
    return dict(codes=np.full(2 * W - 2, ONE, np.uint32), u=np.zeros((ac, W - 1), F32))


def codes_of(a, ceiling) -> np.ndarray:
    """code(a) of float32 magnitudes a."""
    a, c = np.asarray(a, F32), F32(ceiling)
    with np.errstate(all="ignore"):
        v = ((c / a).astype(F32) * F32(16777216.0)).astype(F32)
        over = np.where((a > c) & (a < F32(np.inf)), v, F32(0.0))          # NaN and infinity: 0
    return np.where(a <= c, np.uint32(ONE), over.astype(np.uint32)).astype(np.uint32)


def walk(x, gain0, gain1, W: int, ceiling, state: dict):
    """One channel, one call: x [ac, n] float32, the ramp's end points, state from fresh_state() or the last call ->
    (y [ac, n], the new state, min_code, limited)."""
    x = np.asarray(x, F32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    ac, n = x.shape
    assert W in LOOKAHEADS and n >= 1
    gain0, gain1 = F32(gain0), F32(gain1)
    with np.errstate(all="ignore"):
        stp = F32(F32(gain1 - gain0) * F32(1.0 / n))
        g = fmaf((np.arange(n, dtype=np.int64) + 1).astype(F32), stp, gain0)
        u = (x * g[None, :]).astype(F32)
        q = codes_of(np.abs(u), ceiling).min(axis=0)
        qq = np.concatenate([state["codes"], q])
        mm = np.lib.stride_tricks.sliding_window_view(qq, W).min(axis=1)                       # m[-(W-1) .. n)
        s = (np.lib.stride_tricks.sliding_window_view(mm.astype(np.uint64), W).sum(axis=1) >> np.uint64(W.bit_length() - 1))
        assert len(s) == n and int(s.max()) <= ONE
        sf = (s.astype(F32) * F32(2.0 ** -24)).astype(F32)
        uu = np.concatenate([state["u"], u], axis=1)
        y = (uu[:, :n] * sf[None, :]).astype(F32)
    new = dict(codes=qq[len(qq) - (2 * W - 2):].copy(), u=uu[:, uu.shape[1] - (W - 1):].copy())
    return y, new, int(s.min()), int(np.count_nonzero(s < ONE))


def apply(status, audio, W: int, ceiling, states: list):
    """status: STATUS_DTYPE [N] after the call's control step; audio [N, ac, n]; states: one per channel, replaced -> (the
    output, the status with min_code and limited filled in)."""
    x = np.asarray(audio, F32)
    out, st = np.empty_like(x), np.array(status, STATUS_DTYPE)
    for i in range(x.shape[0]):
        out[i], states[i], st["min_code"][i], st["limited"][i] = walk(x[i], st["gain0"][i], st["gain1"][i], W, ceiling, states[i])
    return out, st


def interleave(audio):
    """[N, ac, n] -> [N, n, ac], the PCM's order."""
    return np.ascontiguousarray(np.transpose(np.asarray(audio), (0, 2, 1)))


def special_rows(rng, ac: int, n: int, W: int, T: int, scale=0.3) -> np.ndarray:
    """[ac, n] float32: noise of `scale` with over-ceiling bursts at the call's and the tile's first and last samples (so that
    a burst's look-ahead crosses a tile and a call boundary), a lone over-ceiling sample, a NaN and an infinity."""
    x = (scale * rng.standard_normal((ac, n))).astype(F32)
    for k in (0, 1, n - 1, T - 1, T, 2 * T - 1, 2 * T):
        if 0 <= k < n:
            x[rng.integers(ac), k] = F32(rng.choice([-1.0, 1.0]) * rng.uniform(2.0, 9.0))
    if n > 4 * W:
        x[:, n // 2:n // 2 + 3] = F32(3.5)                   # both rows together
        x[rng.integers(ac), n // 3] = F32(np.nan)
        x[rng.integers(ac), (2 * n) // 3] = F32(-np.inf if n % 2 else np.inf)
    return x
