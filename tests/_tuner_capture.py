"""Wide captures for the tuner tests: several FM stations at distinct offsets in one u8 I/Q stream (plain numpy)."""
from __future__ import annotations

import numpy as np

import rds_groups as RG

# ---- three stations carrying one audio tone each (selectivity, the float64 bound) -------------------------------------
TONES = dict(Fs_w=19.2e6, R=8, T=64, cutoff=600e3, offsets=(-3.1e6, 0.4e6, 5.2e6), amplitudes=(0.25, 0.25, 0.25),
             tones=(1000.0, 2500.0, 4000.0))


def tone_capture(n_wide: int) -> np.ndarray:
    """u8 I,Q [2 n_wide]: station k = a 75 kHz-deviation FM carrier at offsets[k] modulated by a sine of tones[k] Hz."""
    c = TONES
    n = np.arange(n_wide, dtype=np.float64)
    z = np.zeros(n_wide, np.complex128)
    for f_c, a, f_t in zip(c["offsets"], c["amplitudes"], c["tones"]):
        phi = 2 * np.pi * f_c * n / c["Fs_w"] - 75e3 / f_t * np.cos(2 * np.pi * f_t * n / c["Fs_w"])
        z += a * np.exp(1j * phi)
    iq = np.empty(2 * n_wide, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * z.real + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * z.imag + 0.5), 0, 255)
    return iq


# ---- three stations carrying RDS (capture -> tuner -> stereo bank -> RDS bank) ----------------------------------------
RDS = dict(Fs_w=9.6e6, R=4, T=32, cutoff=600e3, offsets=(-2.3e6, 0.7e6, 3.1e6), amplitudes=(0.28, 0.25, 0.22),
           pi=(0xC201, 0xD318, 0xE42A), ps=("FIRST FM", "SECONDFM", "THIRD FM"), calls=40, bytes_per_call=192000)
assert all(len(p) == 8 for p in RDS["ps"])


def rds_gain(k: int) -> float:
    return 0.8 / RDS["amplitudes"][k]


def rds_capture() -> np.ndarray:
    """u8 I,Q of 1.6 s at 9.6 MS/s: station k's multiplex is rds_groups.station_demod at the wide rate, frequency-modulated
    with the deviation of rds_groups.station_iq_u8 scaled to the wide rate, on a carrier at offsets[k]."""
    c = RDS
    n_wide = c["calls"] * c["bytes_per_call"] // 2 * c["R"]
    n = np.arange(n_wide, dtype=np.float64)
    zr, zi = np.zeros(n_wide), np.zeros(n_wide)
    for k, (f_c, a) in enumerate(zip(c["offsets"], c["amplitudes"])):
        x = RG.station_demod(n_wide, if_Fs=c["Fs_w"], pi=c["pi"][k], ps=c["ps"][k], chip_offset=600 * 40 * (1 + 0.3 * k), seed=k + 1)
        phi = np.cumsum(x.astype(np.float64) / (10.0 * c["R"])) + 2 * np.pi * f_c * n / c["Fs_w"]
        del x
        zr += a * np.cos(phi)
        zi += a * np.sin(phi)
        del phi
    iq = np.empty(2 * n_wide, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * zr + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * zi + 0.5), 0, 255)
    return iq
