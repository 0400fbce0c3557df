"""The three-station RDS capture of tests/_tuner_capture.py re-made as a signed 16-bit capture at 10 MS/s, the rate an Airspy
R2 or an SDRplay delivers: a rational tuner at 6/25 brings it to the banks' 2.4 MS/s (plain numpy)."""
from __future__ import annotations

import numpy as np

import _tuner_capture as TC
import rds_groups as RG

RDS = dict(TC.RDS, Fs_w=10e6, U=6, D=25, T=200)
del RDS["R"], RDS["cutoff"]
N_WIDE_PER_CALL = RDS["bytes_per_call"] // 2 // RDS["U"] * RDS["D"]          # 96000 outputs per channel and call = 400000 wide samples
assert N_WIDE_PER_CALL * RDS["U"] == RDS["bytes_per_call"] // 2 * RDS["D"]
# The call from which the CPU statement of capture -> 6/25 model -> bank -> RDS has every station's PI and PS right
# (tests/test_tuner_rational_model_host.py asserts it); the device chain is allowed 4 calls more, as the integer tuner's is.
RIGHT_FROM_CALL = 16


def rds_gain(k: int) -> float:
    return TC.rds_gain(k)


def rds_capture_10ms_s16() -> np.ndarray:
    """int16 I,Q of 1.6 s at 10 MS/s (32767 units per 1.0): station k's multiplex is rds_groups.station_demod at the wide rate,
    frequency-modulated with the deviation of rds_groups.station_iq_u8 scaled to the wide rate, on a carrier at offsets[k]."""
    c = RDS
    n_wide = c["calls"] * N_WIDE_PER_CALL
    ratio = c["D"] / c["U"]                                                  # wide samples per sample at rf_Fs
    n = np.arange(n_wide, dtype=np.float64)
    zr, zi = np.zeros(n_wide), np.zeros(n_wide)
    for k, (f_c, a) in enumerate(zip(c["offsets"], c["amplitudes"])):
        x = RG.station_demod(n_wide, if_Fs=c["Fs_w"], pi=c["pi"][k], ps=c["ps"][k], chip_offset=600 * 40 * (1 + 0.3 * k), seed=k + 1)
        phi = np.cumsum(x.astype(np.float64) / (10.0 * ratio)) + 2 * np.pi * f_c * n / c["Fs_w"]
        del x
        zr += a * np.cos(phi)
        zi += a * np.sin(phi)
        del phi
    iq = np.empty(2 * n_wide, np.dtype("<i2"))
    iq[0::2] = np.clip(np.floor(32767.0 * zr + 0.5), -32768, 32767)
    iq[1::2] = np.clip(np.floor(32767.0 * zi + 0.5), -32768, 32767)
    return iq
