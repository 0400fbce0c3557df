"""The audio spectrum meter's definition (include/fmrx.h: fmrx_audio_spectrum_*), plain numpy, no GPU.
Host code and kernel equal walk() bit for bit (any NaN counting as any other NaN: a NaN's sign and payload are the machine's).

Frames: a row is a stream across calls; frame f covers stream samples 256 f .. 256 f + 255, no overlap, nothing in front of a
fresh stream.  Carried per channel: fill (0 .. 255, one value for both rows) and the fill samples of the open frame per row.
A call of n samples completes F = (fill + n) div 256 frames and leaves (fill + n) mod 256 samples.
Tables (float32; the bits below are the definition, formula() recomputes them): w[j] = 0.5 - 0.5 cos(2 pi j / 256), the periodic
Hann window; C[m] = cos(2 pi m / 256), built from the quarter m = 0 .. 64 by symmetry with C[64] = C[192] = +0.
Per frame and row: xw[j] = x[j] w[j] (one float32 multiply); for bins k = 0 .. 127
  re_k = the fmaf chain over j = 0 .. 255 ascending from +0 of C[(k j) mod 256] xw[j]
  im_k = the same chain with C[(k j - 64) mod 256]
  p_k  = fmaf(im_k, im_k, fl(re_k re_k))
every step rounded once (tests/_fir_model.py's fmaf), denormals kept.
Bands: edges[0 .. B] strictly ascending within 1 .. 128, 1 <= B <= 32; band b covers bins edges[b] .. edges[b+1] - 1; a frame's
band power is the float32 sum of its p_k ascending from +0.
Record per channel and call (AUDIO_SPECTRUM_DTYPE): n, frames, band[2][32] as float64: the call's completed frames form tiles
of TILE = 16 consecutive frames; a tile's sum runs over its frames ascending from +0.0, the call's sum over its tiles ascending
from +0.0."""
from __future__ import annotations

import numpy as np

from _fir_model import fmaf
from _true_peak_model import _db, same  # noqa: F401  (same: bit for bit, any NaN equal to any NaN)

F32, F64 = np.float32, np.float64
FRAME, BINS, TILE, MAX_BANDS = 256, 128, 16, 32
FULL_SCALE = 2.0
NORM = 6144.0                            # 256 * sum(w^2) / 4: a full-scale sine inside a band reads 0 dBFS
DB_MIN = -99.0
DEFAULT_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128)

C_BITS = """
3f800000 3f7fec43 3f7fb10f 3f7f4e6d 3f7ec46d 3f7e1324 3f7d3aac 3f7c3b28 3f7b14be 3f79c79d 3f7853f8 3f76ba07
3f74fa0b 3f731447 3f710908 3f6ed89e 3f6c835e 3f6a09a7 3f676bd8 3f64aa59 3f61c598 3f5ebe05 3f5b941a 3f584853
3f54db31 3f514d3d 3f4d9f02 3f49d112 3f45e403 3f41d870 3f3daef9 3f396842 3f3504f3 3f3085bb 3f2beb4a 3f273656
3f226799 3f1d7fd1 3f187fc0 3f13682a 3f0e39da 3f08f59b 3f039c3d 3efc5d27 3ef15aea 3ee63375 3edae880 3ecf7bca
3ec3ef15 3eb8442a 3eac7cd4 3ea09ae5 3e94a031 3e888e93 3e78cfcc 3e605c13 3e47c5c2 3e2f10a2 3e164083 3dfab273
3dc8bd36 3d96a905 3d48fb30 3cc90ab0 00000000
"""
W_BITS = """
00000000 391de7df 3a1de1c8 3ab19298 3b1dc971 3b766e3c 3bb15502 3bf1360b 3c1d6830 3c470c54 3c758104 3c945f8c
3cb05f55 3ccebb8a 3cef6f7e 3d093b12 3d1be50c 3d2fb2cc 3d44a143 3d5aad38 3d71d344 3d8507ea 3d91af97 3d9edeb5
3dac933b 3dbacb0c 3dc983f7 3dd8bbb7 3de86ff3 3df89e3f 3e04a20e 3e0d2f7d 3e15f61a 3e1ef48b 3e28296d 3e319354
3e3b30ce 3e45005d 3e4f0080 3e592fab 3e638c4c 3e6e14cb 3e78c786 3e81d16d 3e87528b 3e8ce646 3e928bc0 3e98421b
3e9e0875 3ea3ddeb 3ea9c196 3eafb28e 3eb5afe7 3ebbb8b6 3ec1cc0d 3ec7e8fb 3ece0e90 3ed43bd7 3eda6fdf 3ee0a9b2
3ee6e859 3eed2adf 3ef3704d 3ef9b7ab 3f000000 3f03242b 3f0647d9 3f096a90 3f0c8bd3 3f0fab27 3f12c810 3f15e214
3f18f8b8 3f1c0b82 3f1f19f9 3f2223a5 3f25280c 3f2826b9 3f2b1f35 3f2e110a 3f30fbc5 3f33def3 3f36ba20 3f398cdd
3f3c56ba 3f3f174a 3f41ce1e 3f447acd 3f471ced 3f49b415 3f4c3fe0 3f4ebfe9 3f5133cd 3f539b2b 3f55f5a5 3f5842dd
3f5a827a 3f5cb421 3f5ed77d 3f60ec38 3f62f202 3f64e889 3f66cf81 3f68a69f 3f6a6d99 3f6c2429 3f6dca0d 3f6f5f03
3f70e2cc 3f72552d 3f73b5ec 3f7504d3 3f7641af 3f776c4f 3f788484 3f798a24 3f7a7d05 3f7b5d04 3f7c29fc 3f7ce3cf
3f7d8a5f 3f7e1d94 3f7e9d56 3f7f0992 3f7f6237 3f7fa737 3f7fd888 3f7ff622 3f800000
"""

AUDIO_SPECTRUM_DTYPE = np.dtype([("n", "<u8"), ("frames", "<u8"), ("band", "<f8", (2, MAX_BANDS))])
AUDIO_SPECTRUM_STATE_DTYPE = np.dtype([("fill", "<u4"), ("carry", "<f4", (2, FRAME - 1))])
assert AUDIO_SPECTRUM_DTYPE.itemsize == 528 and AUDIO_SPECTRUM_STATE_DTYPE.itemsize == 2044


def _from_bits(text) -> np.ndarray:
    return np.array([int(t, 16) for t in text.split()], np.uint32).view(F32)


def _unfold(c_quarter, w_half):
    """(w[256], C[256]) from C[0 .. 64] and w[0 .. 128]: C[128 - m] = -C[m], C[256 - m] = C[m], C[64] = C[192] = +0;
    w[256 - j] = w[j]."""
    c = np.zeros(FRAME, F32)
    c[:65] = c_quarter
    c[64:129] = -c_quarter[::-1]
    c[64] = 0.0
    c[129:] = c[127:0:-1]
    w = np.zeros(FRAME, F32)
    w[:129] = w_half
    w[129:] = w[127:0:-1]
    return w, c


W, C = _unfold(_from_bits(C_BITS), _from_bits(W_BITS))


def formula():
    """(w[256], C[256]) recomputed: the float64 formulas rounded once, the cosine's quarter unfolded by symmetry."""
    m = np.arange(FRAME + 1, dtype=F64)
    c = np.cos(2.0 * np.pi * m / FRAME).astype(F32)[:65]
    c[64] = 0.0
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * m / FRAME)).astype(F32)[:129]
    return _unfold(c, w)


def direct():
    """(w[256], C[256]) of the float64 formulas at every index, no symmetry: differs from the tables at C[64] and C[192] only."""
    m = np.arange(FRAME, dtype=F64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * m / FRAME)).astype(F32), np.cos(2.0 * np.pi * m / FRAME).astype(F32)


def fresh(n_channels: int) -> np.ndarray:
    return np.zeros(n_channels, AUDIO_SPECTRUM_STATE_DTYPE)


def check_edges(edges=None) -> np.ndarray:
    e = np.array(DEFAULT_EDGES if edges is None else edges, np.int64)
    assert e.ndim == 1 and 2 <= len(e) <= MAX_BANDS + 1 and e[0] >= 1 and e[-1] <= BINS and (np.diff(e) > 0).all(), e
    return e


def bin_powers(frames) -> np.ndarray:
    """frames float32 [..., 256] -> p float32 [..., 128]."""
    x = np.asarray(frames, F32)
    with np.errstate(all="ignore"):
        xw = x * W
        re = np.zeros(x.shape[:-1] + (BINS,), F32)
        im = re.copy()
        k = np.arange(BINS)
        for j in range(FRAME):
            v = xw[..., j:j + 1]
            re = fmaf(C[(k * j) % FRAME], v, re)
            im = fmaf(C[(k * j - 64) % FRAME], v, im)
        return fmaf(im, im, re * re)


def band_powers(p, edges=None) -> np.ndarray:
    """p float32 [..., 128] -> float32 [..., B]: the sum of a band's bins ascending from +0."""
    e = check_edges(edges)
    p = np.asarray(p, F32)
    out = np.zeros(p.shape[:-1] + (len(e) - 1,), F32)
    with np.errstate(all="ignore"):
        for b in range(len(e) - 1):
            acc = np.zeros(p.shape[:-1], F32)
            for k in range(e[b], e[b + 1]):
                acc = acc + p[..., k]
            out[..., b] = acc
    return out


def two_level(bp) -> np.ndarray:
    """bp float32 [F][...] -> float64 [...]: tiles of 16 frames summed ascending from +0.0, then the tiles."""
    total = np.zeros(bp.shape[1:], F64)
    with np.errstate(all="ignore"):
        for t0 in range(0, bp.shape[0], TILE):
            tile = np.zeros(bp.shape[1:], F64)
            for q in range(t0, min(t0 + TILE, bp.shape[0])):
                tile = tile + bp[q].astype(F64)
            total = total + tile
    return total


def walk(rows, state, edges=None):
    """rows float32 [n_channels][audio_channels][n], state AUDIO_SPECTRUM_STATE_DTYPE [n_channels] -> (records
    AUDIO_SPECTRUM_DTYPE [n_channels], the state after the call).  Channels of one fill are walked together."""
    x = np.asarray(rows, F32)
    N, ac, n = x.shape
    assert ac in (1, 2)
    e = check_edges(edges)
    B = len(e) - 1
    rec = np.zeros(N, AUDIO_SPECTRUM_DTYPE)
    rec["n"] = n
    after = np.zeros(N, AUDIO_SPECTRUM_STATE_DTYPE)
    fills = np.asarray(state["fill"]).astype(np.int64)
    for fill in np.unique(fills):
        ch = np.flatnonzero(fills == fill)
        stream = np.concatenate([np.asarray(state["carry"])[ch][:, :ac, :fill], x[ch]], axis=2)
        F, left = divmod(int(fill) + n, FRAME)
        rec["frames"][ch] = F
        if F:
            fr = stream[:, :, :F * FRAME].reshape(len(ch), ac, F, FRAME)
            bp = band_powers(bin_powers(fr), e)                       # [ch][ac][F][B]
            band = rec["band"][ch]
            band[:, :ac, :B] = two_level(np.moveaxis(bp, 2, 0))
            rec["band"][ch] = band
        st = np.zeros(len(ch), AUDIO_SPECTRUM_STATE_DTYPE)
        st["fill"] = left
        st["carry"][:, :ac, :left] = stream[:, :, F * FRAME:]
        after[ch] = st
    return rec, after


def add(a, b):
    """Records of successive calls add."""
    out = np.array(a, AUDIO_SPECTRUM_DTYPE).copy()
    for f in AUDIO_SPECTRUM_DTYPE.names:
        out[f] = a[f] + b[f]
    return out


def band_hz(edges=None, audio_Fs=48000.0) -> np.ndarray:
    """The centre frequency of every band: (edges[b] + edges[b+1] - 1) / 2 bins."""
    e = check_edges(edges).astype(F64)
    return (e[:-1] + e[1:] - 1.0) / 2.0 * (float(audio_Fs) / FRAME)


def derive(rec, audio_channels: int, edges=None, audio_Fs=48000.0, full_scale: float = FULL_SCALE) -> dict:
    """The levels of one record (double arithmetic; fmrx_audio_spectrum_derive is the same): band_dbfs [2][32], total_dbfs [2],
    centroid_hz [2]."""
    e = check_edges(edges)
    B, ac = len(e) - 1, int(audio_channels)
    frames = float(rec["frames"])
    den = NORM * float(full_scale) * float(full_scale)
    fc = band_hz(e, audio_Fs)
    out = dict(band_dbfs=np.full((2, MAX_BANDS), DB_MIN), total_dbfs=np.full(2, DB_MIN), centroid_hz=np.zeros(2))
    if frames <= 0:
        return out
    for r in range(ac):
        total, moment = 0.0, 0.0
        for b in range(B):
            v = float(rec["band"][r][b])
            out["band_dbfs"][r, b] = _db(v / frames, den)
            total += v
            moment += fc[b] * v
        out["total_dbfs"][r] = _db(total / frames, den)
        with np.errstate(all="ignore"):
            out["centroid_hz"][r] = np.float64(moment) / np.float64(total) if total > 0.0 else 0.0
    return out


def special_rows(rng, n_channels: int, ac: int, n: int) -> np.ndarray:
    """Random rows in which +-2.0f, -0 and float32 denormals are scattered."""
    x = (0.6 * rng.standard_normal((n_channels, ac, n))).astype(F32)
    sp = np.array([2.0, -2.0, -0.0, 0.0, 1e-40, -3e-45, 1.17549435e-38, -1e-39], F32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(sp, int(pick.sum()))
    return x
