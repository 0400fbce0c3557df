"""The true-peak meter's definition (include/fmrx.h: fmrx_true_peak_*), plain numpy, no GPU.  Host code
and kernel equal walk() bit for bit (any NaN counting as any other NaN: a NaN's sign and payload are the machine's).

Interpolator: 4x oversampling (ITU-R BS.1770-4 Annex 2), four phases p of 12 taps over x[k-5 .. k+6] for the waveform at
k + p/4.  Phase 0 is the sample itself.  Phases 1 .. 3 are a Kaiser-windowed sinc (beta = 5),
  H[p][j] = sinc(t) I0(5 sqrt(1 - (t/6)^2)) / I0(5),  t = (j - 5) - p/4,
computed in float64 and rounded once to float32; the float32 table H below is the definition (formula() recomputes it).
Groups: the row is a stream across calls with zeros in front of it; when sample i arrives, group k = i - 6 is evaluated:
  v0 = |x[k]|;  for p = 1, 2, 3: acc = +0; for j = 0 .. 11 ascending: acc = fmaf(H[p][j], x[k-5+j], acc); v_p = |acc|
each step rounded once (tests/_fir_model.py's fmaf), float32 denormals kept.  A call of n samples evaluates exactly n groups;
the carried state per row is the last 11 samples (fresh: zeros).
Record per channel and call (TRUE_PEAK_DTYPE; arrays of 2: rows L, R; mono fills index 0): n; over = groups in which any v has
not v <= limit (NaN counts); true_peak = the maximum of all v, taken with v > m (skips NaN); peak = the maximum of v0."""
from __future__ import annotations

import math

import numpy as np

from _fir_model import fmaf

F32 = np.float32
TAPS, CARRY, LATENCY = 12, 11, 6
DB_MIN, DB_MAX = -99.0, 99.0
FULL_SCALE = 2.0
LIMIT = F32(FULL_SCALE * 10.0 ** (-1.0 / 20.0))          # -1 dBTP

_H1 = [-0.00487442082, 0.0147040663, -0.0342647396, 0.0723257735, -0.163275108, 0.896830738, 0.289778441, -0.105972648, 0.0499966145,
       -0.022908682, 0.00887645595, -0.0022687749]
_H2 = [-0.00483739981, 0.0163076762, -0.0397830643, 0.0850367323, -0.184198961, 0.626807153]
# H[p - 1] for p = 1, 2, 3: H[3] is H[1] reversed, H[2] is symmetric
H = np.array([_H1, _H2 + _H2[::-1], _H1[::-1]], F32)
H_BITS = ("bb9fb99b 3c70e953 bd0c592f 3d941f89 be273197 3f6596b3 3e945dd7 bdd90830 3d4cc940 bcbbaafd 3c116e8e bb14afba",
          "bb9e830d 3c8597ad bd22f391 3dae27bd be3c9ea7 3f20766f")

TRUE_PEAK_DTYPE = np.dtype([("n", "<u8"), ("over", "<u8", (2,)), ("true_peak", "<f8", (2,)), ("peak", "<f8", (2,))])
TRUE_PEAK_LEVELS_NAMES = ("true_peak_dbtp_l", "true_peak_dbtp_r", "peak_dbfs_l", "peak_dbfs_r", "max_dbtp", "over_fraction")
assert TRUE_PEAK_DTYPE.itemsize == 56


def formula() -> np.ndarray:
    """float32 [3][12] of the float64 formula, with numpy's sinc and I0."""
    j = np.arange(TAPS, dtype=np.float64)
    out = []
    for p in (1, 2, 3):
        t = (j - 5.0) - p / 4.0
        out.append(np.sinc(t) * np.i0(5.0 * np.sqrt(1.0 - (t / 6.0) ** 2)) / np.i0(5.0))
    return np.array(out, np.float64).astype(F32)


def fresh(n_channels: int) -> np.ndarray:
    """The state of n_channels fresh channels: float32 [n_channels][2][11]."""
    return np.zeros((n_channels, 2, CARRY), F32)


def groups(e) -> np.ndarray:
    """e float32 [..., 11 + n]: the carried samples, then the call's -> v float32 [..., n, 4], the four values of the call's n groups."""
    e = np.asarray(e, F32)
    n = e.shape[-1] - CARRY
    v = np.zeros(e.shape[:-1] + (n, 4), F32)
    with np.errstate(all="ignore"):
        v[..., 0] = np.abs(e[..., 5:5 + n])
        for p in range(3):
            acc = np.zeros(e.shape[:-1] + (n,), F32)
            for j in range(TAPS):
                acc = fmaf(H[p, j], e[..., j:j + n], acc)
            v[..., p + 1] = np.abs(acc)
    return v


def walk(rows, state, limit=LIMIT):
    """rows float32 [n_channels][audio_channels][n], state float32 [n_channels][2][11] -> (records TRUE_PEAK_DTYPE [n_channels], the
    state after the call)."""
    x = np.asarray(rows, F32)
    N, ac, n = x.shape
    assert ac in (1, 2)
    limit = F32(limit)
    e = np.concatenate([np.asarray(state, F32)[:, :ac], x], axis=2)
    v = groups(e)                                                  # [N][ac][n][4]
    rec = np.zeros(N, TRUE_PEAK_DTYPE)
    rec["n"] = n
    with np.errstate(all="ignore"):
        rec["over"][:, :ac] = (~(v <= limit)).any(axis=3).sum(axis=2)
        # the maximum taken with v > m from +0: NaN never enters, so it is the maximum of the values that are not NaN
        rec["true_peak"][:, :ac] = np.where(np.isnan(v), F32(0), v).max(axis=(2, 3))
        rec["peak"][:, :ac] = np.where(np.isnan(v[..., 0]), F32(0), v[..., 0]).max(axis=2)
    after = np.asarray(state, F32).copy()
    after[:, :ac] = e[:, :, n:]
    return rec, after


def add(a, b):
    """Records of successive calls: n and over add, the peaks take the maximum."""
    out = np.array(a, TRUE_PEAK_DTYPE).copy()
    for f in TRUE_PEAK_DTYPE.names:
        out[f] = np.fmax(a[f], b[f]) if f in ("true_peak", "peak") else a[f] + b[f]
    return out


def same(a, b) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.names:
        return all(same(a[f], b[f]) for f in a.dtype.names)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = "<u8" if a.dtype.itemsize == 8 else "<u4"
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))))


def _db(num: float, den: float) -> float:
    """10 log10(num / den) clamped to [-99, 99]; -99 where num is not positive (NaN included), 99 where only den is not."""
    if not num > 0.0:
        return DB_MIN
    if not den > 0.0:
        return DB_MAX
    ratio = num / den
    if ratio == 0.0 or math.isinf(ratio):
        return DB_MIN if ratio == 0.0 else DB_MAX
    return min(DB_MAX, max(DB_MIN, 10.0 * math.log10(ratio)))


def derive(rec, audio_channels: int, full_scale: float = FULL_SCALE) -> dict:
    """The levels of one record (double arithmetic; fmrx_true_peak_derive is the same)."""
    n, ac, fs2 = float(rec["n"]), int(audio_channels), float(full_scale) * float(full_scale)
    out = dict.fromkeys(TRUE_PEAK_LEVELS_NAMES, 0.0)
    for r, s in enumerate("lr"):
        tp, pk = float(rec["true_peak"][r]), float(rec["peak"][r])
        out["true_peak_dbtp_" + s] = _db(tp * tp, fs2) if r < ac else DB_MIN
        out["peak_dbfs_" + s] = _db(pk * pk, fs2) if r < ac else DB_MIN
    out["max_dbtp"] = max(out["true_peak_dbtp_l"], out["true_peak_dbtp_r"])
    out["over_fraction"] = (float(rec["over"][0]) + float(rec["over"][1])) / (n * ac) if n > 0 else 0.0
    return out


def special_rows(rng, n_channels: int, ac: int, n: int, limit=LIMIT) -> np.ndarray:
    """Random rows in which +-2.0f, -0, float32 denormals and values at `limit` and one ulp either side are scattered.  The last
    channel but one has a NaN in it; the last one infinities of both signs within one window of 12 samples: the phases read NaN
    (infinity minus infinity, where the two taps have one sign) or infinity there and true_peak reads infinity from phase 0 (where
    there are that many channels and samples)."""
    limit = F32(limit)
    x = (0.6 * rng.standard_normal((n_channels, ac, n))).astype(F32)
    sp = np.array([2.0, -2.0, -0.0, 0.0, 1e-40, -3e-45, 1.17549435e-38, limit, -limit, np.nextafter(limit, F32(0)), np.nextafter(limit, F32(4)),
                   -np.nextafter(limit, F32(4))], F32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(sp, int(pick.sum()))
    if n_channels >= 3:
        x[-2, 0, n // 2] = np.nan
        x[-1, ac - 1, n // 3] = np.inf
        if n // 3 + 4 < n:
            x[-1, ac - 1, n // 3 + 4] = -np.inf
    return x
