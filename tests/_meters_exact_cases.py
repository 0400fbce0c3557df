"""The rows on which tests/test_gpu_meters_exact.py compares meters_mpx_kernel bit for bit with tests/_meters_order_model.py, and
on which tests/test_meters_order_model_host.py shows that the comparison has power (plain numpy; every row is a function of a
fixed seed).  Cases (a) - (d) are those of the GPU test's docstring."""
from __future__ import annotations

import functools
import importlib

import numpy as np

import _meters_model as mm
import _meters_order_model as om

IF_FS = 240000.0
L = mm.SEGMENT
PITCH_EXTRA = 5            # device rows sit at a pitch of n_if + 5 floats
NAN32 = np.float32(np.nan)

# (a) (M, tail): the look-ahead's start, the batch edge, the first reuse of an LDS buffer, and 49 and 75 segments (76 800 samples
# is a receiver bank's call of 8 reference blocks); every tail of 0, 1, 255, 256, 257, 1023 samples occurs
A_CASES = ((1, 1023), (2, 0), (3, 1), (15, 255), (16, 256), (17, 257), (31, 1023), (32, 0), (33, 1), (49, 257), (75, 0))
# (b) channels cycle over 5 or 7 base rows (b_base); two and three batches
B_BASE_CHOICES = (5, 7)
B_LENGTHS = (17 * L + 3, 33 * L)
B_NAN_ROW, B_NAN_AT = 2, 16 * L + 4 * 77 + 1      # base row 2: a NaN in segment 16, the first of the second batch
B_OUTLIER_ROW = 1                                 # base row 1: TAIL_OUTLIER as its second tail sample, where there is a tail
# (c) 17 segments and 7 samples, rows as c_rows says; and the same with a third batch, so that the stale-buffer mutant has a
# segment to act on, where the ordinary row also carries TAIL_OUTLIER (the special rows' sums are NaN, infinite or about 1e79)
C_LENGTHS = (17 * L + 7, 33 * L + 7)
# (d) one bank call of 8 reference blocks
D_CHANNELS, D_BLOCK_BYTES = 5, 8 * 192000
# ... and the same rows once more without their last D_SHORT samples: 74 segments and a tail of 765, which the bank's own length
# (75 segments exactly) does not have.  Discriminator rows are bounded by pi, so nothing like TAIL_OUTLIER can be had; 259 is the
# first of 1, 2, 3, 5, 259, 515, 771, 1023 at which the tail's place shows in a total (sum_x2 of two of the five stand-in rows
# of tests/test_meters_order_model_host.py)
D_SHORT = 259


# Sums of a few hundred float32 values of one size are all but exact in float64, so WHEN a thread's running sums take the tail
# shows in a call's total only by luck (one row in twenty).  One tail sample of 2^20 makes it plain: a thread that starts from
# 2^40 rounds every later square to 2^-12, one that ends with it rounds once.
TAIL_OUTLIER = np.float32(2.0 ** 20)


def uniform_rows(n_rows, n_if, seed):
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (n_rows, n_if)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def a_rows(M, tail):
    x = uniform_rows(2 if M >= 49 else 3, M * L + tail, 7100000 + 1024 * M + tail)
    x.setflags(write=False)
    return x


def b_base(cap):
    """the number of base rows: the grid cap (workgroups) is no multiple of it, so the channels one workgroup walks, cap apart,
    sit on different base rows"""
    return next(b for b in B_BASE_CHOICES if cap % b)


@functools.lru_cache(maxsize=None)
def b_rows(n_base, n_if):
    x = uniform_rows(n_base, n_if, 7200000 + n_base * 100000 + n_if)
    x[B_NAN_ROW, B_NAN_AT] = NAN32
    if n_if % L:
        x[B_OUTLIER_ROW, n_if // L * L + 1] = TAIL_OUTLIER
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def c_rows(n_if):
    """row 0: a NaN in segment 3; row 1: +inf inside segment 16 (not at its first sample) and -inf in the tail; row 2: -0.0,
    float32 subnormals and +-3e38; row 3: ordinary"""
    x = uniform_rows(4, n_if, 7300000 + n_if)
    M = n_if // L
    x[0, 3 * L + 4 * 200 + 2] = NAN32
    x[1, 16 * L + 517] = np.float32(np.inf)
    x[1, M * L + 2] = np.float32(-np.inf)
    k = np.random.default_rng(7300001).choice(n_if, 600, replace=False)
    sub = np.array([1, 2, 3, 0x7FFFFF, 0x400001], np.uint32).view(np.float32)      # subnormals: the smallest, the largest
    x[2, k[:100]] = np.float32(-0.0)
    x[2, k[100:300]] = np.tile(np.concatenate([sub, -sub]), 20)
    x[2, k[300:450]] = np.float32(3e38)
    x[2, k[450:]] = np.float32(-3e38)
    x[2, [1, M * L + 4]], x[2, [2, M * L + 5]], x[2, [3, M * L + 6]] = np.float32(-3e38), sub[0], np.float32(-0.0)   # the first segment, the tail
    if n_if != C_LENGTHS[0]:
        x[3, M * L + 1] = TAIL_OUTLIER
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def d_streams():
    """u8 I,Q [D_CHANNELS][D_BLOCK_BYTES]: the package's synthetic stereo station, every channel at another place of the stream
    and with other noise"""
    synth = importlib.import_module("software-defined-radio_amd.synth")
    iq = np.stack([synth.synth_fm_u8(D_BLOCK_BYTES // 2, seed=0x4D58 + c, start=1000003 * c) for c in range(D_CHANNELS)])
    iq.setflags(write=False)
    return iq


def model(rows, table, mutant=None):
    """[om.mpx_ordered of every row]"""
    re, im = table
    return [om.mpx_ordered(r, re, im, mutant) for r in rows]


def differing_fields(rec, want):
    """names of the compared fields whose bits differ (any NaN equal to any NaN)"""
    g, w = om.bits(rec), om.bits(want)
    return [om.FIELD_OF_BITS[i] for i in np.flatnonzero(g != w)]
