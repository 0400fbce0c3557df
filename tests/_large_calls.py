"""Helpers of tests/test_gpu_large_calls.py: how a result of several gigabytes is checked in a second.

The input of a large call is PERIODIC: a base stream of P bytes (a real FM signal) tiled K times, then a ragged tail that
is a prefix of the base.  Every output of the data-parallel kernels depends only on its input window and on its index
modulo a small tile, so with P a whole number of those tiles the outputs of period k >= 1 equal those of period 1 bit for
bit, and the tail's equal the start of period 1.  A small CONTROL call (3 periods and the tail, checked against the
models) proves that for the kernel and the P in question and supplies periods 0 and 1; the large call is then compared
row by row on the device (check_periodic).  Banks are periodic across channels: channel c carries stream c mod 16
(check_channels).

The rules below are conditions on the shape, not measurements: they make sure that an index wrapped at 2^31 or 2^32 bytes
(of the input or of any checked output) lands on data that DIFFERS from what belongs there.  Everything works on numpy
arrays and on torch tensors alike; tests/test_large_calls_host.py runs the scheme scaled down (boundary 2^20) against
deliberately wrapped indices."""
from __future__ import annotations

import numpy as np

BOUNDARIES = (1 << 31, 1 << 32)     # byte offsets at which a narrowed index wraps
MARGIN = 64 << 20                   # the data reaches this far past the last boundary: more than one batch for each of the
                                    # 2048 waves of the fused kernel's largest grid (2048 x 25 600 = 52 MB)
PIECE = 1024                        # bytes per DMA piece of the matrix-core kernels
F32_SENTINEL = 0x7FC00000           # a NaN: outputs are filled with it before a large call (an unwritten region fails)
S16_SENTINEL = 0x5A5A
GROUP = 16                          # distinct streams of a bank: the fused kernel's chain depends on an output's index
                                    # mod 16 in the pseudo-stream, and a slot need not be a multiple of 16 outputs


class Mismatch(AssertionError):
    """where: 'period' | 'tail' | 'channel'; index: the first bad period / channel (None for the tail); offset: its first
    byte in the checked buffer; bad: every bad period / channel."""

    def __init__(self, msg, where, index, offset, bad):
        super().__init__(msg)
        self.where, self.index, self.offset, self.bad = where, index, offset, bad


# ---- the rules ------------------------------------------------------------------------------------------------------
def periods_needed(P, unit, boundaries=BOUNDARIES, margin=MARGIN, piece=PIECE, scale=(1, 1)):
    """K such that K P scale >= the last boundary + margin (scale: bytes of the buffer that has to cross per input byte as
    a fraction, e.g. (4, 5) for the interleaved IF at decimation 5).  P must be a whole number of the path's largest arithmetic
    unit and of DMA pieces, and must not divide a boundary (a wrapped offset would alias onto identical data)."""
    assert P > 0 and P % unit == 0, f"P = {P} is not a whole number of units of {unit} bytes"
    assert P % piece == 0, f"P = {P} is not a whole number of {piece}-byte DMA pieces"
    for b in boundaries:
        assert b % P != 0, f"P = {P} divides the boundary {b}: a wrapped offset would alias onto identical data"
    need = -(-(max(boundaries) + margin) * scale[1] // scale[0])
    K = -(-need // P)
    assert K * P * scale[0] >= (max(boundaries) + margin) * scale[1] and K >= 4
    return K


def check_tail(tail, P, legal, batch, sixteen):
    """The tail is a legal block length (a multiple of `legal` bytes) shorter than a period that is neither a whole batch
    nor a whole number of 16 audio outputs (`sixteen` bytes of input)."""
    assert 0 < tail < P and tail % legal == 0, f"tail {tail} is not a legal block length (multiples of {legal} below {P})"
    assert tail % batch != 0 and tail % sixteen != 0, f"tail {tail} is a whole number of batches ({batch}) or of 16 outputs ({sixteen})"


def assert_no_alias(name, period1, boundaries=BOUNDARIES, total_bytes=None):
    """For every boundary b: the shift b mod (bytes of a period in this buffer) is not 0, and the period's data shifted
    by it differs from itself in more than half of its elements (covers near-periodic signals).  total_bytes: the size of
    the whole buffer where it is known to end below a boundary -- no offset into it can wrap there, so that boundary
    sets no condition (a bank's outputs: 16 channels x 1024 f32 are 2^16 bytes a period, in a buffer of 0.2 GB)."""
    a = np.ascontiguousarray(period1).ravel()
    nbytes = a.nbytes
    for b in boundaries:
        if total_bytes is not None and total_bytes <= b:
            continue
        shift = b % nbytes
        assert shift != 0, f"{name}: a period of {nbytes} bytes divides the boundary {b}"
        raw = a.view(np.uint8)
        moved = np.roll(raw, -shift).view(a.dtype) if shift % a.itemsize == 0 else None
        if moved is None:      # a shift inside an element: compare as bytes
            differ = float((np.roll(raw, -shift) != raw).mean())
        else:
            differ = float((_bits(moved) != _bits(a)).mean())
        assert differ > 0.5, f"{name}: shifted by {shift} bytes (boundary {b} mod {nbytes}) only {differ:.1%} of a period differs from itself"


# ---- numpy / torch ---------------------------------------------------------------------------------------------------
def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _bits(a):
    """Floats as their bit patterns (NaN sentinels compare equal to themselves, -0.0 differs from +0.0)."""
    if _is_torch(a):
        import torch
        return a.view(torch.int32) if a.dtype == torch.float32 else a
    return a.view(np.int32) if a.dtype == np.float32 else a


def _host(a):
    return a.cpu().numpy() if _is_torch(a) else np.asarray(a)


def _itemsize(a):
    return a.element_size() if _is_torch(a) else a.itemsize


def _flat_nonzero(mask):
    if _is_torch(mask):
        return mask.nonzero().flatten().cpu().numpy()
    return np.flatnonzero(mask)


def _describe(got, want):
    got, want = _bits(np.ascontiguousarray(got)), _bits(np.ascontiguousarray(want))
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}", 0
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if not len(bad):
        return "", None
    return f"{len(bad)} of {got.size} elements differ, first at element {int(bad[0])}", int(bad[0])


def pattern(period1, start, n):
    """n elements of the periodic output from phase `start`: period1[(start + i) mod per]."""
    p = np.asarray(period1)
    return p[(start + np.arange(n)) % len(p)]


# ---- the comparisons -------------------------------------------------------------------------------------------------
def check_periodic(name, out, per, K, want0, want1, in_bytes_per_elem=None):
    """out: 1-d array (device or host) of K periods of `per` elements and a tail.  Periods 0 and 1 must equal want0 / want1
    (the control's) bit for bit, every later period must equal period 1, the tail its prefix of period 1.  The rows are
    compared where the array lives; periods 0 and 1, the tail and the first mismatching period come back to the host.
    Raises Mismatch naming the first bad period, its byte offset in `out` and in the input."""
    tail = out.shape[0] - K * per
    assert out.ndim == 1 and tail >= 0 and len(want0) == per and len(want1) == per, (name, out.shape, K, per)
    size = _itemsize(out)
    b = _bits(out)
    rows = b[:K * per].reshape(K, per)
    bad = (rows != rows[1]).any(1)
    head = _host(rows[:2])
    w = [_bits(np.ascontiguousarray(want0)), _bits(np.ascontiguousarray(want1))]
    bad_periods = [k for k in (0, 1) if not np.array_equal(head[k], w[k])]
    later = _flat_nonzero(bad)
    bad_periods += [int(k) for k in later if k >= 2]
    tl = _host(b[K * per:])
    tail_msg, _ = _describe(tl, w[1][:tail])

    def where(k):
        s = f"period {k} of {K} (byte offset {k * per * size} = {k * per * size:#x} of this buffer"
        if in_bytes_per_elem:
            s += f", {k * per * in_bytes_per_elem} = {k * per * in_bytes_per_elem:#x} of the input"
        return s + ")"

    if bad_periods:
        k = bad_periods[0]
        msg, first = _describe(_host(rows[k]), w[k] if k < 2 else head[1])
        off = (k * per + (first or 0)) * size
        raise Mismatch(f"{name}: {where(k)} differs from {'the control' if k < 2 else 'period 1'}: {msg} (byte offset {off} = {off:#x}); "
                       f"{len(bad_periods)} bad periods, the first few {bad_periods[:8]}" + (f"; tail: {tail_msg}" if tail_msg else ""),
                       "period", k, k * per * size, bad_periods)
    if tail_msg:
        raise Mismatch(f"{name}: the tail of {tail} elements behind {where(K)} differs from the start of period 1: {tail_msg}",
                       "tail", None, K * per * size, [])


def check_channels(name, out, want, group=GROUP, in_pitch=None):
    """out: [N, row] (device or host); channels 0 .. group-1 must equal `want` (the control bank's) bit for bit and channel
    c must equal channel c mod group.  Raises Mismatch naming the first bad channel, its byte offset in `out` and (with
    in_pitch, the bytes between two channels' input slots) in the slots."""
    assert out.ndim == 2 and out.shape[0] >= group and tuple(want.shape) == (group, out.shape[1]), (name, out.shape, want.shape)
    N, row = out.shape
    size = _itemsize(out)
    b = _bits(out)
    q = N // group
    per_ch = (b[:q * group].reshape(q, group, row) != b[:group].reshape(1, group, row)).any(2).reshape(-1)
    bad = [int(c) for c in _flat_nonzero(per_ch)]
    if N > q * group:
        rest = (b[q * group:] != b[:N - q * group]).any(1)
        bad += [q * group + int(c) for c in _flat_nonzero(rest)]
    first = _host(b[:group])
    w = _bits(np.ascontiguousarray(want))
    bad = [c for c in range(group) if not np.array_equal(first[c], w[c])] + [c for c in bad if c >= group]
    if bad:
        c = bad[0]
        msg, _ = _describe(_host(b[c]), w[c] if c < group else first[c % group])
        s = f"channel {c} of {N} (byte offset {c * row * size} = {c * row * size:#x} of this buffer"
        if in_pitch:
            s += f", {c * in_pitch} = {c * in_pitch:#x} of the slots"
        raise Mismatch(f"{name}: {s}) differs from {'the control bank' if c < group else f'channel {c % group}'}: {msg}; "
                       f"{len(bad)} bad channels, the first few {bad[:8]}", "channel", c, c * row * size, bad)
