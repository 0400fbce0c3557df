"""The signal meters' definition (include/fmrx.h: fmrx_meters_*), plain numpy, no GPU.

Per channel and call two groups of raw results, and host arithmetic that turns them into levels.

RF group, from the block's interleaved u8 I,Q bytes (n_iq complex samples, i = I - 128, q = Q - 128), exact integers:
  sum_i, sum_q   sum of i, of q                      m2   sum of p = i^2 + q^2
  m4             sum of p^2 (p <= 2^15)              clipped   bytes equal to 0 or 255
MPX group, from the float32 discriminator row x[0 .. n_if) (radians per IF sample), in float64:
  sum_x, sum_x2, max_abs   over all n_if samples
  probe[p]       sum over the M = n_if // L whole segments (L = 1024) of |sum_k x[sL + k] t_p[k]|^2,
                 t_p[k] = w[k] (cos, -sin)(2 pi f_p k / if_Fs), w[k] = 0.5 - 0.5 cos(2 pi (k + 0.5) / L): Hann-windowed tone
                 powers, averaged incoherently; the phase restarts in every segment because only powers are used
  f_p            17 kHz, 21 kHz (noise, the guard bands beside the pilot), 19 kHz (pilot), 57 kHz -+ 1187.5 Hz (RDS: the
                 biphase spectrum's maxima; it has a null at 57 kHz itself)
mpx_group below is defined for finite rows and adds in numpy's order.  The order in which the device adds, and with it the value
of every float64 bit for bit, is stated by tests/_meters_order_model.py, which also extends the definition to rows that are not
finite: sums and probes follow IEEE arithmetic in that order and may read NaN or infinity; max_abs is the largest |x| among the
samples that are not NaN, 0 if there is none.

Limits of the definition: cnr_db is over the slot's whole bandwidth (rf_Fs), not over the 200 kHz of a channel; and the
noise probes sit 2 kHz = about 8.5 bins from the pilot, so the Hann window's leakage of the pilot into them caps pilot_db
(somewhere above 60 dB) however clean the signal."""
from __future__ import annotations

import math

import numpy as np

SEGMENT = 1024
PROBES_HZ = (17000.0, 21000.0, 19000.0, 55812.5, 58187.5)
P_NOISE_LO, P_NOISE_HI, P_PILOT, P_RDS_LO, P_RDS_HI = range(5)
MIN_IF_FS = 120000.0
DB_MIN, DB_MAX = -99.0, 99.0

METER_DTYPE = np.dtype([("n_iq", "<u8"), ("sum_i", "<i8"), ("sum_q", "<i8"), ("m2", "<u8"), ("m4", "<u8"), ("clipped", "<u8"),
                        ("n_if", "<u8"), ("segments", "<u8"), ("sum_x", "<f8"), ("sum_x2", "<f8"), ("max_abs", "<f8"),
                        ("probe", "<f8", (8,))])
assert METER_DTYPE.itemsize == 152
RF_FIELDS = ("n_iq", "sum_i", "sum_q", "m2", "m4", "clipped")
# The device tests' bound on the float64 sums, relative to sum |terms|: reordering n <= 1e5 float64 terms moves a sum by at most
# n 2^-53 ~ 1e-11 of sum |terms|; a power |c|^2 moves by at most 2 A_s delta with |c| <= A_s = sum_k w[k] |x[sL + k]|.  A factor
# of about 10 is left as room.
REL = 1e-10
LEVEL_NAMES = ("level_dbfs", "cnr_db", "clip_fraction", "dc_i", "dc_q", "freq_offset_hz", "peak_dev_hz", "mpx_rms_hz",
               "pilot_dev_hz", "pilot_db", "rds_db")


def window() -> np.ndarray:
    k = np.arange(SEGMENT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 0.5) / SEGMENT)


def table(if_Fs: float):
    """(re, im) float64 [5][1024]: t_p[k] = w[k] (cos, -sin)(2 pi f_p k / if_Fs)."""
    k = np.arange(SEGMENT, dtype=np.float64)
    w = window()
    re, im = np.empty((len(PROBES_HZ), SEGMENT)), np.empty((len(PROBES_HZ), SEGMENT))
    for p, f in enumerate(PROBES_HZ):
        th = 2.0 * np.pi * f * k / float(if_Fs)
        re[p], im[p] = w * np.cos(th), -(w * np.sin(th))
    return re, im


def rf_group(iq_u8) -> dict:
    """Exact integers of one row of interleaved u8 I,Q bytes (an even count)."""
    b = np.asarray(iq_u8, np.uint8).reshape(-1)
    assert len(b) % 2 == 0
    i, q = b[0::2].astype(np.int64) - 128, b[1::2].astype(np.int64) - 128
    p = i * i + q * q
    return dict(n_iq=len(i), sum_i=int(i.sum()), sum_q=int(q.sum()), m2=int(p.sum()), m4=int((p * p).sum()),
                clipped=int(np.count_nonzero(b == 0) + np.count_nonzero(b == 255)))


def mpx_group(x_f32, if_Fs: float) -> dict:
    """float64 sums of one float32 discriminator row; also `bound`, sum_s A_s^2 with A_s = sum_k w[k] |x[sL + k]|: the scale
    of a probe's rounding error (tests/test_gpu_meters.py)."""
    x = np.asarray(x_f32, np.float32).reshape(-1).astype(np.float64)
    M = len(x) // SEGMENT
    re, im = table(if_Fs)
    seg = x[:M * SEGMENT].reshape(M, SEGMENT)
    cr, ci = seg @ re.T, seg @ im.T                      # [M][5]
    probe = np.zeros(8)
    probe[:len(PROBES_HZ)] = (cr * cr + ci * ci).sum(axis=0)
    A = np.abs(seg) @ window()
    return dict(n_if=len(x), segments=M, sum_x=float(x.sum()), sum_x2=float((x * x).sum()),
                max_abs=float(np.abs(x).max()) if len(x) else 0.0, probe=probe, bound=float((A * A).sum()),
                sum_abs=float(np.abs(x).sum()))


def record(iq_u8=None, x_f32=None, if_Fs: float = 240000.0) -> np.ndarray:
    """One METER_DTYPE record; a missing input leaves its group zero with n_iq / n_if = 0."""
    r = np.zeros((), METER_DTYPE)
    if iq_u8 is not None:
        for k, v in rf_group(iq_u8).items():
            r[k] = v
    if x_f32 is not None:
        g = mpx_group(x_f32, if_Fs)
        for k in ("n_if", "segments", "sum_x", "sum_x2", "max_abs", "probe"):
            r[k] = g[k]
    return r


def _db(num: float, den: float) -> float:
    """10 log10(num / den) clamped to [-99, 99]; -99 where num is not positive (0 / 0 included), 99 where only den is not."""
    if not num > 0.0:
        return DB_MIN
    if not den > 0.0:
        return DB_MAX
    ratio = num / den
    if ratio == 0.0 or math.isinf(ratio):          # under- or overflow of the quotient: log10 gives -inf / +inf, clamped
        return DB_MIN if ratio == 0.0 else DB_MAX
    return min(DB_MAX, max(DB_MIN, 10.0 * math.log10(ratio)))


def _mean(a: float, n: float) -> float:
    return a / n if n > 0 else 0.0


def derive(rec, if_Fs: float) -> dict:
    """The levels of one record (double arithmetic; fmrx_meters_derive is the same)."""
    n_iq, n_if, M = float(rec["n_iq"]), float(rec["n_if"]), float(rec["segments"])
    probe = [float(v) for v in rec["probe"]]
    M2, M4 = _mean(float(rec["m2"]), n_iq), _mean(float(rec["m4"]), n_iq)
    S = math.sqrt(max(0.0, 2.0 * M2 * M2 - M4))
    hz = float(if_Fs) / (2.0 * math.pi)
    noise = (probe[P_NOISE_LO] + probe[P_NOISE_HI]) / 2.0
    return dict(
        level_dbfs=_db(M2, 16384.0),
        cnr_db=_db(S, M2 - S),
        clip_fraction=_mean(float(rec["clipped"]), 2.0 * n_iq),
        dc_i=_mean(float(rec["sum_i"]), n_iq),
        dc_q=_mean(float(rec["sum_q"]), n_iq),
        freq_offset_hz=_mean(float(rec["sum_x"]), n_if) * hz,
        peak_dev_hz=float(rec["max_abs"]) * hz,
        mpx_rms_hz=math.sqrt(_mean(float(rec["sum_x2"]), n_if)) * hz,
        pilot_dev_hz=(4.0 * math.sqrt(_mean(probe[P_PILOT], M)) / SEGMENT) * hz,
        pilot_db=_db(probe[P_PILOT], noise),
        rds_db=_db((probe[P_RDS_LO] + probe[P_RDS_HI]) / 2.0, 9.0 * noise),
    )
