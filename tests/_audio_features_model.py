"""The audio feature frames' definition (include/fmrx.h: fmrx_audio_features_*), plain numpy, no GPU.
Host code and kernel equal walk() bit for bit (any NaN counting as any other NaN: a NaN's sign and payload are the machine's).

Geometry: win (a multiple of 4, 16 .. 1280), hop (1 .. win), n_bins (1 .. min(256, win / 2)), n_mels (1 .. 128), 0 <= f_lo < f_hi
<= audio_Fs / 2.  Tables (float32): what fmrx_audio_features_tables returns is the definition, and walk() takes its tables as an
argument; formula() restates them in numpy float64: w[j] = 0.5 - 0.5 cos(2 pi j / win); C[m] = cos(2 pi m / win) unfolded from its
first quarter with C[win/4] = C[3 win/4] = +0; Slaney mel triangles times 2 / (f[b+2] - f[b]); mel_lo / mel_hi around the positive
weights.
Per frame of the mono mix m (0.5f (L + R) for a stereo channel, row 0 for a mono one): xw[j] = m[j] w[j]; for bins k < n_bins
  re_k = the fmaf chain over j = 0 .. win - 1 ascending from +0 of C[(k j) mod win] xw[j]
  im_k = the same chain with C[(k j - win/4) mod win]
  p_k  = fmaf(im_k, im_k, fl(re_k re_k))
  feat[b] = the fmaf chain over k = mel_lo[b] .. mel_hi[b] - 1 ascending from +0 of mel_w[b][k] p_k
every step rounded once (tests/_fir_model.py's fmaf), denormals kept.
Frames: a row is a stream across calls; frame f covers stream samples f hop .. f hop + win - 1, nothing in front of a fresh
stream.  Carried per channel: fill (0 .. win - 1) and the fill samples of the mono mix.  A call of n samples has T = fill + n,
completes F = 0 frames if T < win, else (T - win) div hop + 1, and carries T - F hop samples."""
from __future__ import annotations

import numpy as np

from _fir_model import fmaf
from _true_peak_model import same  # noqa: F401  (bit for bit, any NaN equal to any NaN)

F32, F64 = np.float32, np.float64
MAX_WIN, MAX_BINS, MAX_MELS = 1280, 256, 128
STATE_DTYPE = np.dtype([("fill", "<u4"), ("carry", "<f4", (MAX_WIN - 1,))])
assert STATE_DTYPE.itemsize == 5120

FIELDS = ("win", "hop", "n_bins", "n_mels", "f_lo", "f_hi", "audio_Fs")
G0 = dict(win=64, hop=24, n_bins=24, n_mels=10, f_lo=0.0, f_hi=18000.0, audio_Fs=48000.0)
PRESETS = {48000.0: dict(win=1200, hop=480, n_bins=201, n_mels=80, f_lo=0.0, f_hi=8000.0, audio_Fs=48000.0),
           44100.0: dict(win=1104, hop=441, n_bins=201, n_mels=80, f_lo=0.0, f_hi=8000.0, audio_Fs=44100.0)}


def good(g) -> bool:
    """the geometries the library accepts"""
    win, hop, n_bins, n_mels = (g[k] for k in FIELDS[:4])
    f_lo, f_hi, Fs = (float(g[k]) for k in FIELDS[4:])
    return bool(16 <= win <= MAX_WIN and win % 4 == 0 and 1 <= hop <= win and 1 <= n_bins <= min(MAX_BINS, win // 2) and 1 <= n_mels <= MAX_MELS
                and np.isfinite([f_lo, f_hi, Fs]).all() and 0.0 <= f_lo < f_hi <= Fs / 2.0)


def frames_of(T: int, g) -> int:
    return 0 if T < g["win"] else (T - g["win"]) // g["hop"] + 1


def max_frames(n_audio: int, g) -> int:
    return (n_audio - 1) // g["hop"] + 1


def hz_to_mel(f):
    f = np.asarray(f, F64)
    with np.errstate(all="ignore"):
        return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m):
    m = np.asarray(m, F64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))


def mel_points(g) -> np.ndarray:
    """n_mels + 2 frequencies equally spaced in mel from f_lo to f_hi, float64"""
    lo, hi = float(hz_to_mel(g["f_lo"])), float(hz_to_mel(g["f_hi"]))
    i = np.arange(g["n_mels"] + 2, dtype=F64)
    return mel_to_hz(lo + (hi - lo) * i / (g["n_mels"] + 1))


def filterbank64(g) -> np.ndarray:
    """the Slaney filters in float64 [n_mels][n_bins], not rounded"""
    f = mel_points(g)
    fk = np.arange(g["n_bins"], dtype=F64) * float(g["audio_Fs"]) / g["win"]
    lower = (fk[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - fk[None, :]) / (f[2:] - f[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]


def formula(g) -> dict:
    """The tables restated in numpy: the float64 formulas rounded once, cosine and window unfolded by symmetry."""
    win = g["win"]
    q, h = win // 4, win // 2
    m = np.arange(win + 1, dtype=F64)
    cq = np.cos(2.0 * np.pi * m[:q + 1] / win).astype(F32)
    cq[q] = 0.0
    c = np.zeros(win, F32)
    c[:q + 1] = cq
    c[q:h + 1] = -cq[::-1]
    c[q] = 0.0
    c[h + 1:] = c[h - 1:0:-1]
    w = np.zeros(win, F32)
    w[:h + 1] = (0.5 - 0.5 * np.cos(2.0 * np.pi * m[:h + 1] / win)).astype(F32)
    w[h + 1:] = w[h - 1:0:-1]
    mel_w = filterbank64(g).astype(F32)
    lo, hi = np.zeros(g["n_mels"], np.int32), np.zeros(g["n_mels"], np.int32)
    for b in range(g["n_mels"]):
        k = np.flatnonzero(mel_w[b] > 0)
        if len(k):
            lo[b], hi[b] = k[0], k[-1] + 1
    return dict(window=w, cosine=c, mel_lo=lo, mel_hi=hi, mel_w=mel_w)


def fresh(n_channels: int) -> np.ndarray:
    return np.zeros(n_channels, STATE_DTYPE)


def mono_mix(rows) -> np.ndarray:
    """rows float32 [..., ac, n] -> [..., n]: 0.5f (L + R), or row 0"""
    x = np.asarray(rows, F32)
    with np.errstate(all="ignore"):
        return x[..., 0, :] if x.shape[-2] == 1 else F32(0.5) * (x[..., 0, :] + x[..., 1, :])


def bin_powers(frames, g, t) -> np.ndarray:
    """frames float32 [..., win] of the mono mix -> p float32 [..., n_bins]; vectorised over the bins and whatever stands in front"""
    x = np.asarray(frames, F32)
    win, n_bins = g["win"], g["n_bins"]
    c = np.asarray(t["cosine"], F32)
    with np.errstate(all="ignore"):
        xw = x * np.asarray(t["window"], F32)
        re = np.zeros(x.shape[:-1] + (n_bins,), F32)
        im = re.copy()
        k = np.arange(n_bins)
        for j in range(win):
            v = xw[..., j:j + 1]
            re = fmaf(c[(k * j) % win], v, re)
            im = fmaf(c[(k * j - win // 4) % win], v, im)
        return fmaf(im, im, re * re)


def mel_features(p, g, t) -> np.ndarray:
    """p float32 [..., n_bins] -> float32 [..., n_mels]"""
    p = np.asarray(p, F32)
    out = np.zeros(p.shape[:-1] + (g["n_mels"],), F32)
    with np.errstate(all="ignore"):
        for b in range(g["n_mels"]):
            acc = np.zeros(p.shape[:-1], F32)
            for k in range(int(t["mel_lo"][b]), int(t["mel_hi"][b])):
                acc = fmaf(t["mel_w"][b, k], p[..., k], acc)
            out[..., b] = acc
    return out


def frame_features(frames, g, t) -> np.ndarray:
    return mel_features(bin_powers(frames, g, t), g, t)


def walk(rows, state, g, t):
    """rows float32 [n_channels][audio_channels][n], state STATE_DTYPE [n_channels], the geometry and its tables -> (feat float32
    [n_channels][F_max(n)][n_mels] with the frames a channel did not complete +0, frames uint32 [n_channels], the state after the
    call).  Channels of one fill are walked together."""
    x = np.asarray(rows, F32)
    N, ac, n = x.shape
    assert ac in (1, 2) and good(g)
    win, hop = g["win"], g["hop"]
    m = mono_mix(x)
    feat = np.zeros((N, max_frames(n, g), g["n_mels"]), F32)
    frames = np.zeros(N, np.uint32)
    after = np.zeros(N, STATE_DTYPE)
    fills = np.asarray(state["fill"]).astype(np.int64)
    for fill in np.unique(fills):
        assert fill < win
        ch = np.flatnonzero(fills == fill)
        stream = np.concatenate([np.asarray(state["carry"])[ch][:, :fill], m[ch]], axis=1)
        T = int(fill) + n
        F = frames_of(T, g)
        frames[ch] = F
        if F:
            idx = hop * np.arange(F)[:, None] + np.arange(win)[None, :]
            feat[ch, :F] = frame_features(stream[:, idx], g, t)
        st = np.zeros(len(ch), STATE_DTYPE)
        st["fill"] = T - F * hop
        st["carry"][:, :T - F * hop] = stream[:, F * hop:]
        after[ch] = st
    return feat, frames, after


def special_rows(rng, n_channels: int, ac: int, n: int) -> np.ndarray:
    """Random rows in which +-2.0f, -0 and float32 denormals are scattered."""
    x = (0.6 * rng.standard_normal((n_channels, ac, n))).astype(F32)
    sp = np.array([2.0, -2.0, -0.0, 0.0, 1e-40, -3e-45, 1.17549435e-38, -1e-39], F32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(sp, int(pick.sum()))
    return x
