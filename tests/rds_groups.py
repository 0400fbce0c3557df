"""RDS groups with station data, modulated at a chosen chip rate (test infrastructure for the station decoder).

rds_signal.py sends random information words; a station decoder needs real groups: 0A / 0B (PS name, TA, MS) and 2A / 2B
(RadioText) of one PI and PTY, with their checkwords and offset words (IEC 62106; C' = 0x350 for version-B groups).  The bits
are modulated as rds_signal.rds_demod_signal does (differential encoding, biphase chips, half-sine chip shape on a 57 kHz
subcarrier locked to the pilot, plus a mono programme), with the chip rate as an argument: a transmitter off by +-150 ppm
exercises the decoder's chip timing.  station_iq_u8 turns the multiplex into u8 I/Q at 2.4 MS/s as _rds_util.rds_iq_u8
does."""
import numpy as np

from rds_signal import OFFSETS, checkword

OFFSET_CP = 0x350                  # offset word C' (version-B groups)


def block_bits(info: int, offset: str) -> list:
    off = OFFSET_CP if offset == "Cp" else OFFSETS[offset]
    word = (info << 10) | (checkword(info) ^ off)
    return [(word >> (25 - k)) & 1 for k in range(26)]


def group_bits(blocks) -> list:
    """blocks: four (info, offset) pairs -> 104 bits."""
    out = []
    for info, off in blocks:
        out += block_bits(info, off)
    return out


def _b_word(gt: int, version: str, tp: int, pty: int, low5: int) -> int:
    return (gt << 12) | ((1 if version == "B" else 0) << 11) | (tp << 10) | (pty << 5) | (low5 & 31)


def _pair(s: bytes, i: int) -> int:
    return (s[i] << 8) | s[i + 1]


def group_0(pi: int, pty: int, ps: str, seg: int, version="A", tp=0, ta=0, ms=1, af=0xE0CD):
    """Group 0A / 0B: two PS characters of segment seg; 0A carries alternative-frequency codes in C, 0B the PI in C'."""
    p = ps.encode("latin-1").ljust(8)[:8]
    b = _b_word(0, version, tp, pty, (ta << 4) | (ms << 3) | (seg & 3))
    c = (af, "C") if version == "A" else (pi, "Cp")
    return [(pi, "A"), (b, "B"), c, (_pair(p, 2 * seg), "D")]


def group_2(pi: int, pty: int, rt: str, seg: int, ab=0, version="A", tp=0):
    """Group 2A (four RadioText characters of segment seg, 64 in all) or 2B (two, 32 in all)."""
    b = _b_word(2, version, tp, pty, (ab << 4) | (seg & 15))
    if version == "A":
        t = rt.encode("latin-1").ljust(64)[:64]
        return [(pi, "A"), (b, "B"), (_pair(t, 4 * seg), "C"), (_pair(t, 4 * seg + 2), "D")]
    t = rt.encode("latin-1").ljust(32)[:32]
    return [(pi, "A"), (b, "B"), (pi, "Cp"), (_pair(t, 2 * seg), "D")]


def station_groups(pi: int, pty: int, ps: str, rt: str, n_groups: int, version="A", rt_version="A", ab=0, tp=0):
    """n_groups groups of one station: 0x (PS segment k % 4) and 2x (the RadioText's segments in turn, as many as its length
    needs) alternately."""
    per = 4 if rt_version == "A" else 2
    n_seg = max(1, -(-len(rt) // per))
    out = []
    for k in range(n_groups):
        if k % 2 == 0:
            out.append(group_0(pi, pty, ps, (k // 2) % 4, version=version, tp=tp))
        else:
            out.append(group_2(pi, pty, rt, (k // 2) % n_seg, ab=ab, version=rt_version, tp=tp))
    return out


def stream_bits(groups) -> np.ndarray:
    bits = []
    for g in groups:
        bits += group_bits(g)
    return np.array(bits, np.uint8)


def modulate(bits, n_samples: int, if_Fs: float = 240e3, chip_rate: float = 2375.0, chip_offset: float = 0.0, amplitude: float = 0.06,
             noise: float = 0.0, seed: int = 1) -> np.ndarray:
    """bits (repeated as needed) -> fm_demod float32[n_samples], as rds_signal.rds_demod_signal modulates them, chips at
    chip_rate (the 57 kHz subcarrier stays locked to the pilot)."""
    bits = np.asarray(bits, np.uint8)
    n_bits = int(np.ceil(n_samples / if_Fs * chip_rate / 2)) + 8
    bits = np.tile(bits, -(-n_bits // len(bits)))
    d = np.bitwise_xor.accumulate(bits).astype(np.int8)            # differential encoding
    chips = np.empty(2 * len(d), np.float64)                          # biphase: 1 -> (+, -), 0 -> (-, +)
    chips[0::2] = np.where(d == 1, 1.0, -1.0)
    chips[1::2] = -chips[0::2]
    t = np.arange(n_samples, dtype=np.float64) / if_Fs
    pos = (np.arange(n_samples) - chip_offset) * (chip_rate / if_Fs)
    idx = np.clip(np.floor(pos).astype(np.int64), 0, len(chips) - 1)
    frac = pos - np.floor(pos)
    base = chips[idx] * np.sin(np.pi * frac)
    pilot_phase = 2 * np.pi * 19e3 * t + 0.3
    mono = 0.25 * np.cos(2 * np.pi * 1e3 * t) + 0.15 * np.cos(2 * np.pi * 2.5e3 * t)
    x = mono + 0.1 * np.cos(pilot_phase) + amplitude * base * np.cos(3 * pilot_phase)
    if noise:
        x = x + noise * np.random.default_rng(seed + 99).standard_normal(n_samples)
    return x.astype(np.float32)


def station_demod(n_samples: int, pi=0xC201, pty=10, ps="TESTFM  ", rt="HELLO RDS WORLD!", if_Fs=240e3, chip_rate=2375.0,
                  chip_offset=0.0, amplitude=0.06, noise=0.0, seed=1, version="A", rt_version="A", ab=0) -> np.ndarray:
    """fm_demod of one station transmitting PI, PTY, PS and RadioText over and over."""
    per = 4 if rt_version == "A" else 2
    n_seg = max(1, -(-len(rt) // per))
    groups = station_groups(pi, pty, ps, rt, 2 * max(4, n_seg) * 2, version=version, rt_version=rt_version, ab=ab)
    return modulate(stream_bits(groups), n_samples, if_Fs, chip_rate, chip_offset, amplitude, noise, seed)


def station_iq_u8(n_rf: int, **kw) -> np.ndarray:
    """u8 I/Q at 2.4 MS/s (n_rf complex samples) of an FM transmitter whose multiplex is station_demod(...) at the RF rate."""
    x = station_demod(n_rf, if_Fs=2.4e6, **kw)
    phi = np.cumsum(x.astype(np.float64) / 10.0)
    iq = np.empty(2 * n_rf, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * 0.8 * np.cos(phi) + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * 0.8 * np.sin(phi) + 0.5), 0, 255)
    return iq
