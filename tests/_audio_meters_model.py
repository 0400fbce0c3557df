"""The audio meters' definition (include/fmrx.h: fmrx_audio_meters_*, fmrx_loudness_*), plain numpy,
no GPU.  Host code and kernel equal walk() bit for bit (any NaN counting as any other NaN: a NaN's sign and payload are the
machine's).

K-weighting (ITU-R BS.1770-4's pre-filter, designed for the row's audio_Fs): two biquads in float64, K = tan(pi f0 / Fs),
KQ = K / Q, K2 = K K, a0 = (1 + KQ) + K2:
  shelf      f0 = 1681.974450955533, Q = 0.7071752369554196, Vh = 10^(3.999843853973347 / 20), Vb = Vh^0.4996667741545416
             (both written as literals);
             b = [((Vh + Vb KQ) + K2) / a0, (2 (K2 - Vh)) / a0, ((Vh - Vb KQ) + K2) / a0]
             a = [(2 (K2 - 1)) / a0, ((1 - KQ) + K2) / a0]
  high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1] (not normalised, as the standard's table); a as above
Walk, per row and sample x (float32), v = (double)x, for each biquad in turn (transposed direct form II; every step one IEEE
double operation, no fused multiply-add, denormals kept):
  o = b0 v + z1;  z1 = (b1 v - a1 o) + z2;  z2 = b2 v - a2 o
Record per channel and call (AUDIO_METER_DTYPE; arrays of 2: rows L, R; mono fills index 0): n; over = samples with
not |x| < 2 (NaN counts); peak = max |x| (skips NaN); sum_x, sum_x2, sum_k2 = sum y^2 (y the K-weighted sample), sum_lr =
sum L R (0 for mono): float64, serial in sample order; bins_done.
100 ms bins: bin_len = floor(audio_Fs / 10 + 0.5); after each sample y^2 is added to bin_acc[r]; when bin_fill reaches bin_len,
bin_acc[r] goes to bins[r][bins_done] and is cleared.  State per channel (carried across calls): z[2][4], bin_acc[2], bin_fill.
Gated loudness (BS.1770-4): blocks of 4 consecutive bins, hop one bin, rows summed; see gated()."""
from __future__ import annotations

import math

import numpy as np

VH = 1.5848647011308556
VB = 1.2587209302325617
SHELF_F0, SHELF_Q = 1681.974450955533, 0.7071752369554196
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773
DB_MIN, DB_MAX = -99.0, 99.0
FULL_SCALE = 2.0
ABS_GATE, REL_GATE, OFFSET = -70.0, -10.0, -0.691
BLOCK_BINS, SHORT_BINS = 4, 30

AUDIO_METER_DTYPE = np.dtype([("n", "<u8"), ("over", "<u8", (2,)), ("peak", "<f8", (2,)), ("sum_x", "<f8", (2,)), ("sum_x2", "<f8", (2,)),
                              ("sum_k2", "<f8", (2,)), ("sum_lr", "<f8"), ("bins_done", "<u8")])
AUDIO_LEVELS_NAMES = ("peak_dbfs_l", "peak_dbfs_r", "rms_dbfs_l", "rms_dbfs_r", "dc_l", "dc_r", "loudness_lkfs", "correlation",
                      "balance_db", "over_fraction")
assert AUDIO_METER_DTYPE.itemsize == 104


def design(Fs: float) -> np.ndarray:
    """float64 [2][5]: (b0, b1, b2, a1, a2) of the shelf and of the high-pass."""
    Fs = float(Fs)
    K = math.tan(math.pi * SHELF_F0 / Fs)
    KQ, K2 = K / SHELF_Q, K * K
    a0 = (1.0 + KQ) + K2
    shelf = [((VH + VB * KQ) + K2) / a0, (2.0 * (K2 - VH)) / a0, ((VH - VB * KQ) + K2) / a0, (2.0 * (K2 - 1.0)) / a0, ((1.0 - KQ) + K2) / a0]
    K = math.tan(math.pi * HP_F0 / Fs)
    KQ, K2 = K / HP_Q, K * K
    a0 = (1.0 + KQ) + K2
    hp = [1.0, -2.0, 1.0, (2.0 * (K2 - 1.0)) / a0, ((1.0 - KQ) + K2) / a0]
    return np.array([shelf, hp], np.float64)


def bin_len(Fs: float) -> int:
    return int(float(Fs) / 10.0 + 0.5)


def max_bins(Fs: float, n_audio: int) -> int:
    return int(n_audio) // bin_len(Fs) + 1


def fresh(n_channels: int) -> dict:
    """The state of n_channels fresh channels."""
    return dict(z=np.zeros((n_channels, 2, 4)), bin_acc=np.zeros((n_channels, 2)), bin_fill=np.zeros(n_channels, np.int64))


def walk(Fs: float, rows, state: dict, n_bins: int | None = None):
    """rows float32 [n_channels][audio_channels][n] -> (records AUDIO_METER_DTYPE [n_channels], bins float64 [n_channels][2][n_bins],
    the state after the call).  n_bins defaults to max_bins(Fs, n); entries past bins_done are 0."""
    x = np.asarray(rows, np.float32)
    N, ac, n = x.shape
    assert ac in (1, 2)
    c = design(Fs)
    L = bin_len(Fs)
    n_bins = max_bins(Fs, n) if n_bins is None else n_bins
    z, acc, fill = state["z"].copy(), state["bin_acc"].copy(), state["bin_fill"].copy()
    rec = np.zeros(N, AUDIO_METER_DTYPE)
    bins = np.zeros((N, 2, n_bins))
    done = np.zeros(N, np.int64)
    over, peak = np.zeros((N, 2), np.int64), np.zeros((N, 2), np.float32)
    sx, sx2, sk2, slr = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N)
    idx = np.arange(N)
    with np.errstate(all="ignore"):
        for k in range(n):
            for r in range(ac):
                xf = x[:, r, k]
                a = np.abs(xf)
                over[:, r] += ~(a < np.float32(2.0))
                peak[:, r] = np.where(a > peak[:, r], a, peak[:, r])
                v = xf.astype(np.float64)
                sx[:, r] = sx[:, r] + v
                sx2[:, r] = sx2[:, r] + v * v
                for q in range(2):
                    b0, b1, b2, a1, a2 = c[q]
                    z1, z2 = z[:, r, 2 * q], z[:, r, 2 * q + 1]
                    o = b0 * v + z1
                    z[:, r, 2 * q] = (b1 * v - a1 * o) + z2
                    z[:, r, 2 * q + 1] = b2 * v - a2 * o
                    v = o
                y2 = v * v
                sk2[:, r] = sk2[:, r] + y2
                acc[:, r] = acc[:, r] + y2
            if ac == 2:
                slr = slr + x[:, 0, k].astype(np.float64) * x[:, 1, k].astype(np.float64)
            fill += 1
            closed = fill == L
            if closed.any():
                w = idx[closed]
                bins[w, :, done[w]] = acc[w]
                acc[w] = 0.0
                fill[w] = 0
                done[w] += 1
    rec["n"], rec["over"], rec["peak"], rec["sum_x"], rec["sum_x2"], rec["sum_k2"], rec["sum_lr"], rec["bins_done"] = n, over, peak, sx, sx2, sk2, slr, done
    return rec, bins, dict(z=z, bin_acc=acc, bin_fill=fill)


def add(a, b):
    """Records of successive calls: every field adds, peak takes the maximum."""
    out = np.array(a, AUDIO_METER_DTYPE).copy()
    for f in AUDIO_METER_DTYPE.names:
        out[f] = np.fmax(a[f], b[f]) if f == "peak" else a[f] + b[f]
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


def _db(num: float, den: float, offset: float = 0.0) -> float:
    """offset + 10 log10(num / den) clamped to [-99, 99]; -99 where num is not positive (0 / 0 and NaN included), 99 where only den
    is not."""
    if not num > 0.0:
        return DB_MIN
    if not den > 0.0:
        return DB_MAX
    ratio = num / den
    if ratio == 0.0 or math.isinf(ratio):
        return DB_MIN if ratio == 0.0 else DB_MAX
    return min(DB_MAX, max(DB_MIN, offset + 10.0 * math.log10(ratio)))


def derive(rec, audio_channels: int, full_scale: float = FULL_SCALE) -> dict:
    """The levels of one record (double arithmetic; fmrx_audio_meters_derive is the same)."""
    n, ac, fs2 = float(rec["n"]), int(audio_channels), float(full_scale) * float(full_scale)
    out = dict.fromkeys(AUDIO_LEVELS_NAMES, 0.0)
    for r, s in enumerate("lr"):
        live = r < ac
        p, x2 = float(rec["peak"][r]), float(rec["sum_x2"][r])
        out["peak_dbfs_" + s] = _db(p * p, fs2) if live else DB_MIN
        out["rms_dbfs_" + s] = _db(x2 / n if n > 0 else 0.0, fs2) if live else DB_MIN
        out["dc_" + s] = float(rec["sum_x"][r]) / n if live and n > 0 else 0.0
    k2 = float(rec["sum_k2"][0]) + (float(rec["sum_k2"][1]) if ac == 2 else 0.0)
    out["loudness_lkfs"] = _db(k2 / n if n > 0 else 0.0, fs2, OFFSET)
    if ac == 2:
        den = math.sqrt(float(rec["sum_x2"][0]) * float(rec["sum_x2"][1]))
        out["correlation"] = float(rec["sum_lr"]) / den if den > 0.0 and math.isfinite(den) else 0.0
        out["balance_db"] = _db(float(rec["sum_x2"][0]), float(rec["sum_x2"][1]))
    out["over_fraction"] = (float(rec["over"][0]) + float(rec["over"][1])) / (n * ac) if n > 0 else 0.0
    return out


def gated(bins, Fs: float, full_scale: float = FULL_SCALE, max_blocks: int | None = None) -> dict:
    """bins: float64 [2][m] (or [m], rows already summed): every bin of one channel so far, in order -> momentary (the last
    block), short_term (the last 30 bins), integrated (BS.1770-4: blocks of 4 bins, hop 1; absolute gate -70 LKFS; relative gate
    10 LU under the loudness of the mean of the absolutely gated blocks), blocks, full.  -99 where there is nothing to read."""
    e = np.asarray(bins, np.float64)
    e = e if e.ndim == 1 else e[0] + e[1]
    L, fs2 = bin_len(Fs), float(full_scale) * float(full_scale)
    lk = lambda z: _db(z, 1.0, OFFSET)
    m = len(e)
    nb = max(0, m - BLOCK_BINS + 1)
    full = max_blocks is not None and nb >= max_blocks
    if max_blocks is not None:
        nb = min(nb, max_blocks)
    z = np.array([((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3] for j in range(nb)]) / (BLOCK_BINS * L) / fs2
    out = dict(momentary=DB_MIN, short_term=DB_MIN, integrated=DB_MIN, blocks=nb, full=bool(full))
    if m >= BLOCK_BINS:
        out["momentary"] = lk((((e[m - 4] + e[m - 3]) + e[m - 2]) + e[m - 1]) / (BLOCK_BINS * L) / fs2)
    if m >= SHORT_BINS:
        s = 0.0
        for v in e[m - SHORT_BINS:]:
            s = s + v
        out["short_term"] = lk(s / (SHORT_BINS * L) / fs2)
    t_abs = 10.0 ** ((ABS_GATE - OFFSET) / 10.0)
    ga = z[z > t_abs]
    if len(ga):
        s = 0.0
        for v in ga:
            s = s + v
        t_rel = (s / len(ga)) * 10.0 ** (REL_GATE / 10.0)
        gr = ga[ga > t_rel]
        if len(gr):
            s = 0.0
            for v in gr:
                s = s + v
            out["integrated"] = lk(s / len(gr))
    return out


def special_rows(rng, n_channels: int, ac: int, n: int) -> np.ndarray:
    """Random rows in which +-2.0f, values beyond it, -0 and float32 denormals are scattered; the last channel but one is a row with
    a NaN in it, the last one a row with an infinity (where there are that many channels)."""
    x = (0.6 * rng.standard_normal((n_channels, ac, n))).astype(np.float32)
    sp = np.array([2.0, -2.0, 2.5, -3.0, np.float32(2.0) - np.float32(2.0 ** -22), -0.0, 0.0, 1e-40, -3e-45, 1.17549435e-38], np.float32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(sp, int(pick.sum()))
    if n_channels >= 3:
        x[-2, 0, n // 2] = np.nan
        x[-1, ac - 1, n // 3] = np.inf
    return x


def walk_scalar(Fs: float, x, state: dict):
    """walk() for one mono row in Python floats (IEEE doubles, one operation per step), for the long rows the vectorised loop is
    too slow for; finite input only.  state: dict(z=[4 floats], bin_acc=float, bin_fill=int) -> (dict(sum_x, sum_x2, sum_k2,
    bins_done), the bins [max_bins] with 0 past bins_done, the state after)."""
    (s0, s1, s2, s3, s4), (h0, h1, h2, h3, h4) = (tuple(float(v) for v in q) for q in design(Fs))
    z0, z1, z2, z3 = (float(v) for v in state["z"])
    acc, fill, L = float(state["bin_acc"]), int(state["bin_fill"]), bin_len(Fs)
    sx = sx2 = sk2 = 0.0
    bins = []
    for v in np.asarray(x, np.float32).astype(np.float64).tolist():
        sx = sx + v
        sx2 = sx2 + v * v
        o = s0 * v + z0
        z0 = (s1 * v - s3 * o) + z1
        z1 = s2 * v - s4 * o
        y = h0 * o + z2
        z2 = (h1 * o - h3 * y) + z3
        z3 = h2 * o - h4 * y
        y2 = y * y
        sk2 = sk2 + y2
        acc = acc + y2
        fill += 1
        if fill == L:
            bins.append(acc)
            acc, fill = 0.0, 0
    done = len(bins)
    bins += [0.0] * (max_bins(Fs, len(x)) - done)
    return dict(sum_x=sx, sum_x2=sx2, sum_k2=sk2, bins_done=done), bins, dict(z=[z0, z1, z2, z3], bin_acc=acc, bin_fill=fill)
