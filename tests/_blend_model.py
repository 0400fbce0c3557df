"""The stereo blend / soft mute stage's definition (include/fmrx.h: fmrx_blend_*), plain numpy, no GPU.
The host function (fmrx_blend_control) and both kernels equal this file bit for bit.

Control, float64, per channel and call, from the MPX group of the channel's meter record (probe[0 .. 5), segments).  Every
step is one IEEE operation, in the order written; no fused multiply-add, no sqrt, no log.

    noise = (probe[17k] + probe[21k]) * 0.5
    d_p = drive(probe[19k], noise)                  the pilot ratio
    d_q = drive(ref1 * segments, noise)             quieting; ref1 = w * w, w = ((2 pi * 7500) / if_Fs) * 256
    drive(num, den): -inf where not num > 0; else +inf where not den > 0; else r = num / den: -inf where not r > 0, +inf
                     where r is infinite, else plog2(r) = (e - 1) + (2 f - 1) with (f, e) = frexp(r)  [Mitchell: e + (m - 1)]
    thresholds: dB / 3.010299956639812; ramp(d; lo, hi) = clamp((d - lo) * (1 / (hi - lo)), 0, 1), clamp(x) = 0 where x < 0, 1 where x > 1
    lamp = 1 where d_p >= pilot_on, 0 where d_p < pilot_off, else as it was (0 on a first call)
    t_b = ramp(d_p; blend_lo, blend_hi) where the lamp is on, else 0;   t_m = floor + (1 - floor) * ramp(d_q; mute_lo, mute_hi)
    first call after create / reset: s = t; else v = s + c * (t - s), c = attack where t < s else release; s = t where |t - v| <= 2^-10 else v
    mono1 = float32(1 - s_b), gain1 = float32(s_m); mono0, gain0 = the previous call's mono1, gain1 (a first call: this call's)

Apply, float32, sample k of the call's n:

    a[k] = clamp(fmaf(float32(k + 1), (mono1 - mono0) * inv_n, mono0)), inv_n = float32(1.0 / n); m[k] the same from gain0, gain1
    D = 0.5 * (L - R);  l = L where a[k] == 0 else fmaf(-a[k], D, L);  r = R where a[k] == 0 else fmaf(a[k], D, R)
    L' = m[k] * l, R' = m[k] * r;   mono rows: x' = m[k] * x

Two floats are "the same" when their bits are equal or both are NaN (_deemph_model.same)."""
from __future__ import annotations

import math

import numpy as np

from _deemph_model import same  # noqa: F401  (the tests' comparison)
from _fir_model import fmaf

F32, F64 = np.float32, np.float64
DB_PER_OCTAVE = 3.010299956639812
SNAP = 2.0 ** -10
P_NOISE_LO, P_NOISE_HI, P_PILOT = 0, 1, 2
PLOG2_ERROR = 0.0861            # max of log2(m) - (m - 1) on [1, 2): 0.08607 at m = 1 / ln 2

DEFAULTS = dict(pilot_on=20.0, pilot_off=14.0, blend_lo=20.0, blend_hi=32.0, mute_lo=10.0, mute_hi=24.0, mute_floor=0.0,
                attack=1.0, release=0.25)
PARAM_NAMES = tuple(DEFAULTS)
STATUS_DTYPE = np.dtype([("pilot_db", "<f8"), ("quiet_db", "<f8"), ("sep_target", "<f8"), ("gain_target", "<f8"), ("sep", "<f8"),
                         ("gain", "<f8"), ("mono0", "<f4"), ("gain0", "<f4"), ("mono1", "<f4"), ("gain1", "<f4"), ("lamp", "<u4"),
                         ("reserved", "<u4"), ("calls", "<u8")])
assert STATUS_DTYPE.itemsize == 80


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def valid(p: dict, if_Fs: float) -> bool:
    v = [float(p[k]) for k in PARAM_NAMES]
    if not all(math.isfinite(x) for x in v) or not (math.isfinite(if_Fs) and if_Fs > 0):
        return False
    return (p["blend_hi"] > p["blend_lo"] and p["mute_hi"] > p["mute_lo"] and p["pilot_on"] >= p["pilot_off"]
            and 0.0 <= p["mute_floor"] <= 1.0 and 0.0 < p["attack"] <= 1.0 and 0.0 < p["release"] <= 1.0)


def control(p: dict, if_Fs: float) -> dict:
    """The parameters as the step uses them (blend::Control)."""
    assert valid(p, if_Fs)
    c = dict(pilot_on=p["pilot_on"] / DB_PER_OCTAVE, pilot_off=p["pilot_off"] / DB_PER_OCTAVE, blend_lo=p["blend_lo"] / DB_PER_OCTAVE,
             mute_lo=p["mute_lo"] / DB_PER_OCTAVE, floor=float(p["mute_floor"]), one_minus_floor=1.0 - p["mute_floor"],
             attack=float(p["attack"]), release=float(p["release"]))
    c["blend_inv"] = 1.0 / (p["blend_hi"] / DB_PER_OCTAVE - c["blend_lo"])
    c["mute_inv"] = 1.0 / (p["mute_hi"] / DB_PER_OCTAVE - c["mute_lo"])
    w = ((2.0 * 3.14159265358979323846 * 7500.0) / float(if_Fs)) * 256.0
    c["ref1"] = w * w
    return c


def plog2(r: float) -> float:
    f, e = math.frexp(r)
    return float(e - 1) + (2.0 * f - 1.0)


def drive(num: float, den: float) -> float:
    if not num > 0.0:
        return -math.inf
    if not den > 0.0:
        return math.inf
    r = float(F64(num) / F64(den))          # numpy: infinity and 0 instead of Python's exceptions
    if not r > 0.0:
        return -math.inf
    if math.isinf(r):
        return math.inf
    return plog2(r)


def ramp(d: float, lo: float, inv_span: float) -> float:
    x = (d - lo) * inv_span
    return 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)


def smooth(s: float, t: float, first: bool, c: dict) -> float:
    if first:
        return t
    k = c["attack"] if t < s else c["release"]
    v = s + k * (t - s)
    return t if abs(t - v) <= SNAP else v


def fresh(n=None) -> np.ndarray:
    return np.zeros(() if n is None else n, STATUS_DTYPE)


def step(c: dict, rec, st) -> np.ndarray:
    """One channel's control step: c from control(), rec a meter record (probe, segments), st a STATUS_DTYPE scalar ->
    the new one."""
    with np.errstate(all="ignore"):
        probe = [float(v) for v in rec["probe"]]
        noise = float((F64(probe[P_NOISE_LO]) + F64(probe[P_NOISE_HI])) * F64(0.5))
        dp = drive(probe[P_PILOT], noise)
        dq = drive(float(F64(c["ref1"]) * F64(float(int(rec["segments"])))), noise)
        first = int(st["calls"]) == 0
        kept = 0 if first else int(st["lamp"])
        lamp = 1 if dp >= c["pilot_on"] else (0 if dp < c["pilot_off"] else kept)
        tb = ramp(dp, c["blend_lo"], c["blend_inv"]) if lamp else 0.0
        tm = c["floor"] + c["one_minus_floor"] * ramp(dq, c["mute_lo"], c["mute_inv"])
        sb, sm = smooth(float(st["sep"]), tb, first, c), smooth(float(st["gain"]), tm, first, c)
        mono1, gain1 = F32(1.0 - sb), F32(sm)
        out = np.zeros((), STATUS_DTYPE)
        out["mono0"], out["gain0"] = (mono1, gain1) if first else (st["mono1"], st["gain1"])
        out["mono1"], out["gain1"] = mono1, gain1
        out["pilot_db"], out["quiet_db"] = F64(dp) * F64(DB_PER_OCTAVE), F64(dq) * F64(DB_PER_OCTAVE)
        out["sep_target"], out["gain_target"], out["sep"], out["gain"] = tb, tm, sb, sm
        out["lamp"], out["calls"] = lamp, int(st["calls"]) + 1
    return out


def step_all(c: dict, recs, state) -> np.ndarray:
    return np.array([step(c, recs[i], state[i]) for i in range(len(recs))], STATUS_DTYPE)


def _clamp01(x):
    return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


def ramps(v0, v1, n):
    """[rows, n] float32: value k of each row's ramp from v0 to v1 across n samples."""
    v0, v1 = np.atleast_1d(np.asarray(v0, F32)), np.atleast_1d(np.asarray(v1, F32))
    inv_n = F32(1.0 / n)
    st = ((v1 - v0).astype(F32) * inv_n).astype(F32)
    k1 = (np.arange(n, dtype=np.int64) + 1).astype(F32)
    return _clamp01(fmaf(k1[None, :], st[:, None], v0[:, None]))


def apply_gains(a, m, audio):
    """a, m: [N, n] float32 (or broadcastable); audio [N, ac, n] float32 -> the same shape."""
    x = np.asarray(audio, F32)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        a = np.broadcast_to(np.asarray(a, F32), x[:, 0].shape)
        m = np.broadcast_to(np.asarray(m, F32), x[:, 0].shape)
        if x.shape[1] == 1:
            out[:, 0] = (m * x[:, 0]).astype(F32)
            return out
        L, R = x[:, 0], x[:, 1]
        D = (F32(0.5) * (L - R).astype(F32)).astype(F32)
        l = np.where(a == 0, L, fmaf(-a, D, L)).astype(F32)
        r = np.where(a == 0, R, fmaf(a, D, R)).astype(F32)
        out[:, 0], out[:, 1] = (m * l).astype(F32), (m * r).astype(F32)
    return out


def apply(status, audio):
    """status: STATUS_DTYPE [N] after the call's control step; audio [N, ac, n]."""
    n = np.asarray(audio).shape[2]
    return apply_gains(ramps(status["mono0"], status["mono1"], n), ramps(status["gain0"], status["gain1"], n), audio)


def interleave(audio):
    """[N, ac, n] -> [N, n, ac], the PCM's order."""
    return np.ascontiguousarray(np.transpose(np.asarray(audio), (0, 2, 1)))


def rec_for(c, pilot_d, quiet_d, segments=9, exact=None) -> np.ndarray:
    """A meter record (tests/_meters_model.METER_DTYPE) whose drives are pilot_d and quiet_d (pseudo-log2: dB /
    DB_PER_OCTAVE): both noise probes ref1 * segments / r_q (their mean is exact), pilot = noise * r_p, r = ratio_of(d).
    exact = "pilot" / "quiet": that drive equals the wanted one bit for bit.  A rounded quotient does not reach every double, so
    the search walks the doubles next to the operand it may move, and then the other freedom it has: the noise (pilot) or
    the number of segments (quiet); the other drive is then only close."""
    import _meters_model as mm
    r = np.zeros((), mm.METER_DTYPE)
    noise = pilot = None
    if exact == "quiet":
        for seg in range(segments, segments + 64):
            ref = c["ref1"] * seg
            noise = _near(ref / ratio_of(quiet_d), lambda x: drive(ref, x) == quiet_d)
            if noise is not None:
                segments = seg
                break
        assert noise is not None, "no record gives the quieting drive %r" % quiet_d
    else:
        noise = c["ref1"] * segments / ratio_of(quiet_d)
    if exact == "pilot":
        for _ in range(64):
            pilot = _near(noise * ratio_of(pilot_d), lambda x: drive(x, noise) == pilot_d)
            if pilot is not None:
                break
            noise = math.nextafter(noise, math.inf)
        assert pilot is not None, "no record gives the pilot drive %r" % pilot_d
    else:
        pilot = noise * ratio_of(pilot_d)
    r["segments"], r["n_if"] = segments, segments * mm.SEGMENT
    r["probe"][P_NOISE_LO] = r["probe"][P_NOISE_HI] = noise
    r["probe"][P_PILOT] = pilot
    return r


def _near(x0: float, hit):
    lo = hi = x0
    for _ in range(8):
        if hit(lo):
            return lo
        if hit(hi):
            return hi
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
    return None


def ratio_of(d: float) -> float:
    """The r with plog2(r) = d where d's fraction has the bits to spare: (1 + frac) * 2^floor(d)."""
    e = math.floor(d)
    return math.ldexp(1.0 + (d - e), e)


# ---- what the tests feed: hand-made records, call sequences, audio rows ----------------------------------------------
def _meter_dtype():
    import _meters_model as mm
    return mm.METER_DTYPE


def rec(probe=(0, 0, 0, 0, 0), segments=9):
    r = np.zeros((), _meter_dtype())
    r["probe"][:5] = probe
    r["segments"], r["n_if"] = segments, segments * 1024
    return r


def hand_made_records():
    sub = 5e-324
    return {
        "all zero": rec(),
        "noise 0, pilot > 0": rec((0, 0, 3.0, 0, 0)),
        "pilot 0": rec((2e-3, 4e-3, 0.0, 0, 0)),
        "a station": rec((2e-3, 4e-3, 50.0, 0.9, 1.1)),
        "NaN pilot": rec((2e-3, 4e-3, math.nan, 0, 0)),
        "NaN noise": rec((math.nan, 4e-3, 50.0, 0, 0)),
        "infinite pilot": rec((2e-3, 4e-3, math.inf, 0, 0)),
        "infinite noise": rec((math.inf, 4e-3, 50.0, 0, 0)),
        "infinite both": rec((math.inf, math.inf, math.inf, 0, 0)),
        "negative noise": rec((-1.0, -2.0, 50.0, 0, 0)),
        "subnormal powers": rec((3 * sub, 5 * sub, 1000 * sub, 0, 0)),
        "subnormal noise, ordinary pilot": rec((sub, sub, 1.0, 0, 0)),
        "ordinary noise, subnormal pilot": rec((1.0, 1.0, 7 * sub, 0, 0)),
        "quotient overflows": rec((1e-200, 1e-200, 1e200, 0, 0)),
        "quotient underflows": rec((1e200, 1e200, 1e-200, 0, 0)),
        "segments 0": rec((2e-3, 4e-3, 50.0, 0, 0), segments=0),
        "one segment": rec((2e-3, 4e-3, 50.0, 0, 0), segments=1),
    }


PARAM_SETS = {"defaults": {}, "floor and slow": dict(mute_floor=0.25, attack=0.5, release=0.125),
              "narrow": dict(pilot_on=15.0, pilot_off=15.0, blend_lo=10.0, blend_hi=11.0, mute_lo=-3.0, mute_hi=40.0)}


def sequences(c):
    """name -> list of records, or None = reset before the next one.  Drives in dB."""
    def r(pilot_db, quiet_db=40.0):
        return rec_for(c, pilot_db / DB_PER_OCTAVE, quiet_db / DB_PER_OCTAVE)
    return {
        "hysteresis": [r(22), r(17), r(13), r(17), r(21)],
        "attack and release": [r(40), r(21)] + [r(40)] * 26,       # release 0.25: 0.75^k <= 2^-10 from k = 25
        "mute and recover": [r(40, 30), r(40, 5)] + [r(40, 30)] * 26,
        "partial": [r(26, 17), r(29, 20), r(23, 14), r(26, 17)],
        "reset": [r(40), r(10, 5), None, r(40), r(26, 17), None, r(10, 5), r(40)],
    }


def random_rows(rng, N, ac, n):
    """normal x 0.4 with a few samples beyond +-2, some +-0, NaN and +-inf"""
    x = (0.4 * rng.standard_normal((N, ac, n))).astype(F32)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)
    k = max(1, flat.size // 50)
    for j, v in enumerate((2.5, -3.0, 0.0, -0.0, math.nan, math.inf, -math.inf, 1e-40, 70000.0, -140000.0)):
        flat[idx[j * k:(j + 1) * k][:max(1, k // 3)]] = v
    return x
