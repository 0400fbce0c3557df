"""RDS groups beyond PS and RadioText, and exact bit errors (test infrastructure for the station decoder's correction and its
extension record; rds_groups.py stays the maker of 0A / 0B / 2A / 2B and the modulator).

Groups: 4A (clock time), 1A (variant 0: extended country code, variant 3: language; the programme item number in D), 10A
(programme type name), 0A with a chosen pair of alternative-frequency codes and a decoder-identification bit.
station_schedule cycles 0A x 4, 2A x n, 1A, 1A, 4A, 10A x 2.  with_errors XORs a pattern onto the transmitted bits:
rds_groups.modulate encodes them differentially and the receiver decodes differentially, so one flipped input bit is exactly
one wrong bit at the receiver, a run of flipped bits exactly that burst.  (Give modulate a stream at least as long as the
signal: it tiles shorter ones, and the patterns would repeat with them.)"""
import numpy as np

import rds_groups as RG
from rds_groups import _b_word, _pair


def group_4a(pi, pty, mjd, hour, minute, offset, tp=0):
    """Clock time: MJD (17 bits), UTC hour and minute, offset = the raw 6 bits (bit 5: sign, bits 4..0: half hours)."""
    b = _b_word(4, "A", tp, pty, (mjd >> 15) & 3)
    c = ((mjd & 0x7FFF) << 1) | ((hour >> 4) & 1)
    d = ((hour & 15) << 12) | ((minute & 63) << 6) | (offset & 63)
    return [(pi, "A"), (b, "B"), (c, "C"), (d, "D")]


def group_1a(pi, pty, variant, value, pin, tp=0):
    """Slow labelling codes: variant 0 carries the extended country code (8 bits), variant 3 the language (12 bits)."""
    b = _b_word(1, "A", tp, pty, 0)
    c = ((variant & 7) << 12) | (value & 0xFFF)
    return [(pi, "A"), (b, "B"), (c, "C"), (pin, "D")]


def group_10a(pi, pty, ptyn, seg, ab=0, tp=0):
    t = ptyn.encode("latin-1").ljust(8)[:8]
    b = _b_word(10, "A", tp, pty, (ab << 4) | (seg & 1))
    return [(pi, "A"), (b, "B"), (_pair(t, 4 * seg), "C"), (_pair(t, 4 * seg + 2), "D")]


def group_0a(pi, pty, ps, seg, af_pair, di=0, tp=0, ta=0, ms=1):
    """0A with the two alternative-frequency codes af_pair = (high byte, low byte) and the decoder-identification bit that
    goes with segment seg: bit 3 - seg of the 4-bit word di."""
    p = ps.encode("latin-1").ljust(8)[:8]
    dbit = (di >> (3 - (seg & 3))) & 1
    b = _b_word(0, "A", tp, pty, (ta << 4) | (ms << 3) | (dbit << 2) | (seg & 3))
    return [(pi, "A"), (b, "B"), ((af_pair[0] << 8) | af_pair[1], "C"), (_pair(p, 2 * seg), "D")]


def af_code(mhz: float) -> int:
    return int(round((mhz - 87.5) * 10))


def station_schedule(pi, pty, ps, rt, n_cycles=1, af=(), di=0, ecc=0xE0, lang=0x009, pin=0x1234, ct=(60000, 12, 30, 0), ptyn="PTYNAME ",
                     ptyn_ab=0, rt_ab=0):
    """n_cycles of: 0A x 4 (the PS name; C carries the count code 224 + len(af), then the frequencies af in MHz pairwise, the
    filler 205 where they run out), 2A x n (the RadioText's segments), 1A variant 0, 1A variant 3, 4A, 10A x 2.
    ct = (mjd, hour, minute, raw offset)."""
    codes = [224 + len(af)] + [af_code(f) for f in af]
    codes += [205] * (8 - len(codes)) if len(codes) <= 8 else []
    assert len(codes) == 8, "at most 7 alternative frequencies fit the four 0A groups of a cycle"
    n_seg = max(1, -(-len(rt) // 4))
    out = []
    for _ in range(n_cycles):
        for seg in range(4):
            out.append(group_0a(pi, pty, ps, seg, (codes[2 * seg], codes[2 * seg + 1]), di=di))
        for seg in range(n_seg):
            out.append(RG.group_2(pi, pty, rt, seg, ab=rt_ab))
        out.append(group_1a(pi, pty, 0, ecc, pin))
        out.append(group_1a(pi, pty, 3, lang, pin))
        out.append(group_4a(pi, pty, *ct))
        out.append(group_10a(pi, pty, ptyn, 0, ab=ptyn_ab))
        out.append(group_10a(pi, pty, ptyn, 1, ab=ptyn_ab))
    return out


def cycle_groups(rt) -> int:
    """Groups in one cycle of station_schedule."""
    return 4 + max(1, -(-len(rt) // 4)) + 5


def with_errors(bits, pattern) -> np.ndarray:
    """bits ^ pattern (pattern shorter than bits: the rest stays clean)."""
    bits = np.array(bits, np.uint8)
    pattern = np.asarray(pattern, np.uint8)
    n = min(len(bits), len(pattern))
    bits[:n] ^= pattern[:n] & 1
    return bits


def burst_pattern(n_bits, every_blocks=3, length=2, first_block=1, at=7, inner=None):
    """An error pattern for a stream of n_bits that starts on a block boundary: one burst of `length` bits in every
    `every_blocks`-th block from block first_block on, its first bit at bit `at` of the block (at + length > 26 straddles
    into the next block).  inner: the bits between the two ends, default all wrong."""
    p = np.zeros(n_bits, np.uint8)
    burst = np.ones(length, np.uint8)
    if inner is not None and length > 2:
        burst[1:-1] = inner
    for blk in range(first_block, n_bits // 26, every_blocks):
        lo = 26 * blk + at
        k = min(length, n_bits - lo)
        if k > 0:
            p[lo:lo + k] ^= burst[:k]
    return p
