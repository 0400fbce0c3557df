"""The three-station RDS capture of tests/_tuner_capture.py re-made as a signed 16-bit capture with every amplitude divided
by 128: the stations sit where an 8-bit capture no longer sees them (its u8 quantisation is within +-1 LSB of 128), an S16
tuner with the gains times 128 tunes them to the same level as before (plain numpy)."""
from __future__ import annotations

import numpy as np

import _tuner_capture as TC
import rds_groups as RG

DOWN = 128.0


def rds_gain_s16(k: int) -> float:
    return TC.rds_gain(k) * DOWN


def rds_capture_s16(also_u8=False):
    """int16 I,Q of 1.6 s at 9.6 MS/s (32767 units per 1.0): _tuner_capture.rds_capture's signal, amplitudes / 128.
    also_u8: -> (int16, the same signal quantised to u8 as that file does it)."""
    c = TC.RDS
    n_wide = c["calls"] * c["bytes_per_call"] // 2 * c["R"]
    n = np.arange(n_wide, dtype=np.float64)
    zr, zi = np.zeros(n_wide), np.zeros(n_wide)
    for k, (f_c, a) in enumerate(zip(c["offsets"], c["amplitudes"])):
        x = RG.station_demod(n_wide, if_Fs=c["Fs_w"], pi=c["pi"][k], ps=c["ps"][k], chip_offset=600 * 40 * (1 + 0.3 * k), seed=k + 1)
        phi = np.cumsum(x.astype(np.float64) / (10.0 * c["R"])) + 2 * np.pi * f_c * n / c["Fs_w"]
        del x
        zr += a / DOWN * np.cos(phi)
        zi += a / DOWN * np.sin(phi)
        del phi
    iq = np.empty(2 * n_wide, np.dtype("<i2"))
    iq[0::2] = np.clip(np.floor(32767.0 * zr + 0.5), -32768, 32767)
    iq[1::2] = np.clip(np.floor(32767.0 * zi + 0.5), -32768, 32767)
    if not also_u8:
        return iq
    u8 = np.empty(2 * n_wide, np.uint8)
    u8[0::2] = np.clip(np.floor(128.0 + 127.0 * zr + 0.5), 0, 255)
    u8[1::2] = np.clip(np.floor(128.0 + 127.0 * zi + 0.5), 0, 255)
    return iq, u8
