"""Shared by the RDS tests (test_gpu_rds.py, test_gpu_rds_bank.py, test_gpu_rds_station.py, test_rds_bank_host.py): the
comparisons and the makers of discriminator streams and I/Q.  Needs no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BLOCK = 9600                     # IF samples per call: the receiver banks' block_bytes 192 000 at rf_decim 10
N = 70                           # a full wave of lanes and a partial one
SILENT, LATE = 5, 9               # station_rows: the channel without a signal, the one whose signal starts late
SMALL = (240000, 151, 1, 1, 26, 101)   # RdsParams without rate change: any block of at least 150 samples is legal


def ht(a, n=256):
    return a if len(a) <= 2 * n else np.concatenate([a[:n], a[-n:]])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), msg


def rds_iq_u8(n_blocks, seed=5, amplitude=0.06, chip_offset=600.0):
    """u8 I/Q at 2.4 MS/s of an FM transmitter whose multiplex carries RDS: rds_demod_signal sampled at the RF rate is the
    phase increment per IF sample, so a tenth of it per RF sample; 192 000 bytes per block.  -> (iq, transmitted bits)."""
    from rds_signal import rds_demod_signal
    n_rf = BLOCK * 10 * n_blocks
    x, bits = rds_demod_signal(n_rf, 2.4e6, seed=seed, amplitude=amplitude, chip_offset=chip_offset)
    phi = np.cumsum(x.astype(np.float64) / 10.0)
    iq = np.empty(2 * n_rf, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * 0.8 * np.cos(phi) + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * 0.8 * np.sin(phi) + 0.5), 0, 255)
    return iq, bits


def bank_streams(n_blocks, n=N, block=BLOCK):
    """n discriminator streams: different seeds, chip offsets, amplitudes and noise; channel 5 all zeros, channel 9 zeros
    for the first two and a half blocks, then signal."""
    from rds_signal import rds_demod_signal
    rows = []
    for c in range(n):
        x, _ = rds_demod_signal(n_blocks * block, 240e3, seed=100 + c, amplitude=0.03 + 0.01 * (c % 7), chip_offset=float((37 * c) % 101),
                                noise=0.002 * (c % 4))
        rows.append(x)
    rows = np.stack(rows)
    rows[5] = 0.0
    rows[9, :5 * block // 2] = 0.0
    return rows


def channel_station(c):
    return dict(pi=0x1000 + 37 * c, pty=c % 32, ps=f"ST{c:03d}  ".ljust(8)[:8], rt=f"CHANNEL {c} RADIOTEXT"[:20])


def station_rows(n_blocks, n=N):
    """n stations, each with its own PI, PS, RT, amplitude, noise and chip offset (and chip rate); SILENT all zeros; LATE
    zeros for the first 5.5 calls."""
    import rds_groups as RG
    rows = []
    for c in range(n):
        s = channel_station(c)
        rows.append(RG.station_demod(n_blocks * BLOCK, amplitude=0.04 + 0.01 * (c % 5), noise=0.002 * (c % 4), chip_offset=float((53 * c) % 211),
                                     chip_rate=2375.0 * (1 + (c % 7 - 3) * 40e-6), seed=300 + c, **s))
    rows = np.stack(rows)
    rows[SILENT] = 0.0
    rows[LATE, :11 * BLOCK // 2] = 0.0
    return rows
