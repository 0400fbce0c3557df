"""The audio rate converter's definition (include/fmrx.h: fmrx_audio_resample_*), plain numpy, no GPU.  The
host walk and the kernel equal walk() bit for bit (any NaN counting as any other NaN: a NaN's sign and payload are the machine's).

Geometry: a dict of FIELDS: up 1 .. 160, down 1 .. 1024, coprime; taps T, a multiple of 4 within 8 .. 256 with up T <= 16 384; mix 0 or
1; 0 < cutoff <= 1; 0 <= beta <= 20.  preset(audio_Fs, out_Fs) restates fmrx_audio_resample_preset: up / down = out / in reduced, T = 4
ceil(24 / min(1, up / down) / 4), cutoff 0.9, beta 8.
Taps: float32 [up][T], made by the library in double and rounded once; walk() takes the table as an argument (what
fmrx_audio_resample_taps returns is the definition), formula() restates it in numpy float64: with L = up T, c = (L - 1) / 2, w =
cutoff min(1, up / down), g[k] = w sinc(w (k - c) / up) I0(beta sqrt(1 - ((k - c) / (L / 2))^2)) / I0(beta), h[p][j] = g[j up + p].
Input: with mix one row per channel, 0.5f (L + R) for a stereo channel (one float32 add, an exact halving), row 0 for a mono one;
without it every row by itself.  R = 1 with mix, else audio_channels.
An output: a row is a stream across calls with zeros in front of it.  A call brings n inputs; pos (0 .. down - 1) is the position of
its first output in units of 1 / up input sample from its first sample.  Output q has t = pos + q down, i = t div up, p = t mod up and
  y = acc = +0;  for j = 0 .. T - 1 ascending: acc = fmaf(h[p][j], x[i - j], acc)
each step rounded once (tests/_fir_model.py's fmaf), float32 denormals kept.  The call completes M = ceil((n up - pos) / down) outputs
if n up > pos, else 0, and leaves pos' = pos + M down - n up.  The state (STATE_DTYPE) is pos and per converted row the last T - 1
samples, oldest first; the rest of carry reads 0.  Python integers carry the positions: n up exceeds 2^32 at the limits."""
from __future__ import annotations

import math

import numpy as np

from _fir_model import fmaf

F32, F64 = np.float32, np.float64
FIELDS = ("up", "down", "taps", "mix", "cutoff", "beta")
STATE_DTYPE = np.dtype([("pos", "<u4"), ("reserved", "<u4"), ("carry", "<f4", (2, 255))])
assert STATE_DTYPE.itemsize == 2048

# (audio_Fs, out_Fs) -> (up, down, taps): what the preset must give at least
PRESETS = {(48000, 16000): (1, 3, 72), (48000, 8000): (1, 6, 144), (48000, 24000): (1, 2, 48), (48000, 32000): (2, 3, 36),
           (48000, 44100): (147, 160, 28), (44100, 16000): (160, 441, 68), (44100, 22050): (1, 2, 48), (44100, 48000): (160, 147, 24)}


def geometry(up, down, taps, mix=1, cutoff=0.9, beta=8.0) -> dict:
    return dict(up=int(up), down=int(down), taps=int(taps), mix=int(mix), cutoff=float(cutoff), beta=float(beta))


def preset(audio_Fs: int, out_Fs: int, mix=1) -> dict:
    g = math.gcd(int(out_Fs), int(audio_Fs))
    up, down = int(out_Fs) // g, int(audio_Fs) // g
    taps = 24 if up >= down else 4 * (-(-24 * down // (4 * up)))
    return geometry(up, down, taps, mix)


G_SMALL = geometry(3, 7, 8)             # off the presets: the smallest T, a phase step of 1 (7 mod 3)


def rows_of(g: dict, ac: int) -> int:
    return 1 if g["mix"] else ac


def max_out(n: int, g: dict) -> int:
    return -(-int(n) * g["up"] // g["down"])


def outputs_of(n: int, g: dict, pos: int) -> int:
    nu = int(n) * g["up"]
    return -(-(nu - int(pos)) // g["down"]) if nu > pos else 0


def latency(g: dict) -> float:
    return (g["up"] * g["taps"] - 1) / (2.0 * g["up"])


def prototype(g: dict) -> np.ndarray:
    """float64 [up T]: g[k] of the formula, with numpy's sinc and I0."""
    U, T = g["up"], g["taps"]
    L = U * T
    d = np.arange(L, dtype=F64) - (L - 1) / 2.0
    w = g["cutoff"] * min(1.0, U / g["down"])
    return w * np.sinc(w * d / U) * np.i0(g["beta"] * np.sqrt(1.0 - (d / (L / 2.0)) ** 2)) / np.i0(g["beta"])


def formula(g: dict) -> np.ndarray:
    """float32 [up][T]: h[p][j] = g[j up + p] rounded once."""
    return np.ascontiguousarray(prototype(g).reshape(g["taps"], g["up"]).T).astype(F32)


def fresh(n_channels: int) -> np.ndarray:
    return np.zeros(n_channels, STATE_DTYPE)


def mono_mix(x: np.ndarray) -> np.ndarray:
    """x float32 [..., 2, n] -> [..., 1, n]: one float32 add, then an exact halving."""
    with np.errstate(all="ignore"):
        return (F32(0.5) * (x[..., 0:1, :] + x[..., 1:2, :])).astype(F32)


def converted(rows, g: dict) -> np.ndarray:
    """rows float32 [N][ac][n] -> the rows the converter reads, [N][R][n]."""
    x = np.asarray(rows, F32)
    return mono_mix(x) if g["mix"] and x.shape[1] == 2 else x


def chains(e: np.ndarray, h: np.ndarray, g: dict, pos: int, M: int) -> np.ndarray:
    """e float32 [..., T - 1 + n]: the carried samples, then the call's -> the call's M outputs from position pos, float32 [..., M]."""
    U, D, T = g["up"], g["down"], g["taps"]
    t = int(pos) + np.arange(M, dtype=np.int64) * D
    i, p = t // U + (T - 1), t % U
    acc = np.zeros(e.shape[:-1] + (M,), F32)
    with np.errstate(all="ignore"):
        for j in range(T):
            acc = fmaf(h[p, j], e[..., i - j], acc)
    return acc


def walk(rows, state, g: dict, h: np.ndarray):
    """rows float32 [N][ac][n], state STATE_DTYPE [N], h float32 [up][T] -> (out float32 [N][R][max_out(n)], entries a channel did not
    complete +0; counts uint32 [N]; the state after the call)."""
    x = converted(rows, g)
    N, R, n = x.shape
    T = g["taps"]
    assert h.shape == (g["up"], T) and h.dtype == F32
    out = np.zeros((N, R, max_out(n, g)), F32)
    counts = np.zeros(N, np.uint32)
    after = np.array(state, STATE_DTYPE).copy()
    e = np.concatenate([np.asarray(state["carry"], F32)[:, :R, :T - 1], x], axis=2)
    for pos in np.unique(state["pos"]):                           # channels at one position share their outputs' indices
        assert pos < g["down"]
        sel = np.flatnonzero(state["pos"] == pos)
        M = outputs_of(n, g, int(pos))
        out[sel, :, :M] = chains(e[sel], h, g, int(pos), M)
        counts[sel] = M
        after["pos"][sel] = int(pos) + M * g["down"] - n * g["up"]
    after["carry"][:, :R, :T - 1] = e[:, :, n:]
    return out, counts, after


def reference64(x, h: np.ndarray, g: dict):
    """One fresh row x in float64: zero-stuff by up, convolve with the prototype h[j up + p], take every down-th -> (y float64 [M], the
    bound's sum of |h| |x| per output [M])."""
    U, D, T = g["up"], g["down"], g["taps"]
    x = np.asarray(x, F64)
    proto = np.ascontiguousarray(h.astype(F64).T).reshape(-1)     # g[j U + p]
    z = np.zeros(len(x) * U, F64)
    z[::U] = x
    M = outputs_of(len(x), g, 0)
    y = np.convolve(z, proto)[:len(z)][::D][:M]
    mag = np.convolve(np.abs(z), np.abs(proto))[:len(z)][::D][:M]
    return y, mag


def same(a, b) -> bool:
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.names:
        return all(same(a[f], b[f]) for f in a.dtype.names)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((np.ascontiguousarray(a).view("<u4") == np.ascontiguousarray(b).view("<u4")) | (np.isnan(a) & np.isnan(b))))


SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-45, 1.17549435e-38, np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38], F32)


def special_rows(rng, n_channels: int, ac: int, n: int, T: int) -> np.ndarray:
    """Random rows with +-0 and float32 denormals scattered through them and, per channel, one of +-infinity, NaN and +-FLT_MAX at a
    place of its own: the call's first and last samples, T - 1 and T from either end (the carried window's edges) and the middle."""
    x = (0.6 * rng.standard_normal((n_channels, ac, n))).astype(F32)
    pick = rng.random(x.shape) < 0.15
    x[pick] = rng.choice(SPECIALS[:5], int(pick.sum()))
    places = [0, n - 1, min(T - 1, n - 1), min(T, n - 1), max(n - T, 0), max(n - T + 1, 0), n // 2]
    for c in range(n_channels):
        x[c, c % ac, places[c % len(places)]] = SPECIALS[5 + c % 5]
    return x
