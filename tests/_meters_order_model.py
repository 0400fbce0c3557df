"""The order of meters_mpx_kernel's float64 additions (csrc/kernels_meters.hip), plain numpy, no GPU.

tests/_meters_model.py defines WHAT the MPX group is; this file restates in WHICH ORDER the kernel adds, so that a device record
can be compared as bits.  The library is built with -ffp-contract=off and the kernel spells every fma out, so the source fixes
the order.  For one float32 row x[0 .. n_if), M = n_if // 1024, and the table the library uses (fmrx.metersTable(if_Fs): its
entries, not numpy's cos):

  chain      thread t of 256 owns samples 4t .. 4t+3 of every segment.  Per segment and table row r (0-4 real, 5-9 imaginary
             part of probe r % 5): a = 0.0; for j in 0 .. 3: a = fma(double(x[1024 s + 4t + j]), tab[r][4t + j], a)
  wave       the halving butterfly over the 64 lanes of a wave, for o in (32, 16, 8, 4, 2, 1): v[:o] = v[:o] + v[o:2o]
             (wave_sum10's 13 exchanges give exactly these sums: at every step a lane adds its own and its partner's partial
             sum of the values it keeps, lanes l and l ^ o, and a + b = b + a bit for bit)
  workgroup  ((w0 + w1) + w2) + w3 over the four waves
  probe      probe[p] = probe[p] + (re * re + im * im): two rounded products and one add, segments in rising order from 0.0
  sum_x      per thread, from 0.0: sx = sx + d over its samples, segment by segment and j = 0 .. 3 within one, then the tail
  sum_x2     samples M 1024 + t, + 256, ...; sx2 = fma(d, d, sx2), which is sx2 + d * d because d * d is exact in float64;
             then the same butterfly (lane 0 of the shuffle-down tree) and ((w0 + w1) + w2) + w3
  max_abs    an fmax chain over |d| from 0.0; fmax is exact, so the order does not matter

Rows that are not finite (tests/_meters_model.py is defined for finite rows; this extends it, as include/fmrx.h states it):
sum_x, sum_x2 and the probes follow IEEE arithmetic in the order above and may read NaN or infinity -- a NaN or an infinity in
segment s reaches every probe (all 256 threads' chains meet in the reduction) and both sums; samples of the tail reach the sums
alone.  max_abs is the largest |x| among the samples that are not NaN (infinity for an infinity), 0.0 if there is none: fmax
returns its other operand where one is NaN.  Compared as bits, any NaN equals any NaN (the payload and sign of a NaN that
arithmetic produced are not part of the definition).

`mutant` names one deliberate mistake in the order (MUTANTS); tests/test_meters_order_model_host.py shows that each of them changes
the bits on the rows the device is compared on, i.e. that a kernel with that mistake would fail tests/test_gpu_meters_exact.py."""
from __future__ import annotations

import numpy as np

SEGMENT, THREADS, LANES, PROBES = 1024, 256, 64, 5
BATCH = 16   # segments per barrier; two LDS buffers by batch parity, so a stale buffer holds the segment 32 earlier
FIELDS = ("sum_x", "sum_x2", "max_abs", "probe")
MUTANTS = ("unfused", "butterfly_rising", "waves_pairwise", "segments_reversed", "stale_buffer", "tail_first")

_LOW27 = np.int64((1 << 27) - 1)


def _two_sum(a, b):
    """Knuth: s = fl(a + b) and e with s + e = a + b exactly (no overflow)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma64(d, t, a):
    """fma(d, t, a) in float64 with ONE rounding, elementwise, for d that hold float32 values (24-bit significands: a sample
    converted to double).  t is split into its upper 26 bits and the remaining 27, so both products with d are exact; their
    sum is split into the rounded product and its error (TwoSum); then Boldo and Melquiond's emulation: (th, tl) = TwoSum(a,
    uh), v = tl + ul rounded to odd, result = th + v rounded to nearest.  Exactly rounded for finite operands whose product does not
    overflow and is zero or at least 2^-900 in magnitude (its error term, 105 bits further down, must not underflow; float32
    samples times table entries stay above 2^-200).  Where an operand is not finite, and where the result is a zero (whose
    sign the plain operations get right, the product then being exact), plain IEEE d * t + a."""
    d, t, a = np.broadcast_arrays(np.asarray(d, np.float64), np.asarray(t, np.float64), np.asarray(a, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        plain = d * t + a
        t_hi = (t.view(np.int64) & ~_LOW27).view(np.float64)
        t_lo = t - t_hi
        uh, ul = _two_sum(d * t_hi, d * t_lo)
        th, tl = _two_sum(a, uh)
        v, e = _two_sum(tl, ul)
        # round to odd: where tl + ul is inexact and v's last bit is even, the neighbour on e's side (its last bit is odd)
        vb = v.view(np.int64)
        step = np.where((e > 0.0) == (v > 0.0), 1, -1).astype(np.int64)
        v = np.where((e != 0.0) & ((vb & 1) == 0), vb + step, vb).view(np.float64)
        r = th + v
        finite = np.isfinite(d) & np.isfinite(t) & np.isfinite(a)
        return np.where(finite & (r != 0.0), r, plain)


def _butterfly(v, rising=False):
    """[..., 64] -> [...]: lane 0 of the halving butterfly; rising: the mutant that pairs neighbours first (o = 1 ... 32)."""
    v = np.array(v, np.float64)
    if rising:
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0]
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _waves(w, pairwise=False):
    """[..., 4] -> [...]: ((w0 + w1) + w2) + w3"""
    if pairwise:
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def mpx_ordered(x_f32, re, im, mutant=None) -> dict:
    """-> dict(sum_x, sum_x2, max_abs: float; probe: float64 [8], the last three 0.0) of one float32 row of at least one
    segment, as meters_mpx_kernel adds it.  re, im: float64 [5][1024], the library's table."""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x_f32, np.float32).reshape(-1)
    n, M = len(x), len(x) // SEGMENT
    assert M >= 1
    rising, pairwise = mutant == "butterfly_rising", mutant == "waves_pairwise"
    d = x.astype(np.float64)
    seg = d[:M * SEGMENT].reshape(M, 1, THREADS, 4)                       # [s][.][t][j]
    tab = np.concatenate([np.asarray(re, np.float64), np.asarray(im, np.float64)]).reshape(1, 2 * PROBES, THREADS, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.zeros((M, 2 * PROBES, THREADS))
        for j in range(4):
            a = seg[..., j] * tab[..., j] + a if mutant == "unfused" else fma64(seg[..., j], tab[..., j], a)
        w = _butterfly(a.reshape(M, 2 * PROBES, THREADS // LANES, LANES), rising)   # [s][r][wave]: what a segment leaves in LDS
        if mutant == "stale_buffer":
            w = np.concatenate([w[:2 * BATCH], w[:max(0, M - 2 * BATCH)]])
        c = _waves(w, pairwise)                                                      # [s][r]
        power = c[:, :PROBES] * c[:, :PROBES] + c[:, PROBES:] * c[:, PROBES:]
        probe = np.zeros(8)
        for s in (range(M - 1, -1, -1) if mutant == "segments_reversed" else range(M)):
            probe[:PROBES] = probe[:PROBES] + power[s]
        # the running sums: per thread its samples in the order it meets them, then its share of the tail
        tail = np.full(-(-(n - M * SEGMENT) // THREADS) * THREADS, np.nan)
        tail[:n - M * SEGMENT] = d[M * SEGMENT:]
        tail_ok = np.arange(len(tail)) < n - M * SEGMENT
        steps = [(seg[s, 0, :, j], None) for s in range(M) for j in range(4)]
        tails = [(tail[k:k + THREADS], tail_ok[k:k + THREADS]) for k in range(0, len(tail), THREADS)]
        sx, sx2 = np.zeros(THREADS), np.zeros(THREADS)
        for v, ok in (tails + steps if mutant == "tail_first" else steps + tails):
            if ok is None:
                sx, sx2 = sx + v, sx2 + v * v
            else:
                sx, sx2 = np.where(ok, sx + v, sx), np.where(ok, sx2 + v * v, sx2)
        sum_x = _waves(_butterfly(sx.reshape(THREADS // LANES, LANES), rising), pairwise)
        sum_x2 = _waves(_butterfly(sx2.reshape(THREADS // LANES, LANES), rising), pairwise)
        max_abs = float(np.fmax.reduce(np.abs(d), initial=0.0))
    return dict(sum_x=float(sum_x), sum_x2=float(sum_x2), max_abs=max_abs, probe=probe)


def bits(rec) -> np.ndarray:
    """The compared fields of a record (a dict of mpx_ordered or a METER_DTYPE element) as uint64 [11], every NaN mapped to one
    pattern: field by field what 'equal as bits, any NaN equal to any NaN' compares."""
    v = np.concatenate([[rec["sum_x"], rec["sum_x2"], rec["max_abs"]], np.asarray(rec["probe"], np.float64)]).astype(np.float64)
    b = v.view(np.uint64).copy()
    b[np.isnan(v)] = np.uint64(0x7FF8000000000000)
    return b


FIELD_OF_BITS = ("sum_x", "sum_x2", "max_abs") + tuple(f"probe[{p}]" for p in range(8))
