"""The wide capture of the meters' bank test (tests/test_gpu_meters_bank.py): the three RDS stations of
_tuner_capture.RDS (rds_groups.station_demod, Fs_w = 9.6 MS/s, R = 4) over complex Gaussian noise, three calls long,
and the eight channels tuned into it (plain numpy)."""
from __future__ import annotations

import numpy as np

import _tuner_capture as TC
import rds_groups as RG

CALLS, BYTES_PER_CALL, NOISE_SIGMA, SEED = 3, 192000, 0.02, 4011
MISTUNE_HZ = 20e3
# channels 0-2: the stations; 3: station 1 mistuned so that it sits 20 kHz ABOVE the channel's centre (freq_offset_hz reads the
# station's offset from where the channel is tuned: +20 kHz); 4-7: offsets at least 1 MHz from every station
EMPTY_OFFSETS = (-4.0e6, -0.8e6, 1.9e6, 4.3e6)
EMPTY_GAIN = 0.8 / 0.25


def channels():
    """[(offset in Hz, tuner gain)] of the 8 channels."""
    c = TC.RDS
    ch = [(c["offsets"][k], TC.rds_gain(k)) for k in range(3)]
    ch.append((c["offsets"][1] - MISTUNE_HZ, TC.rds_gain(1)))
    ch += [(f, EMPTY_GAIN) for f in EMPTY_OFFSETS]
    assert all(abs(f - s) >= 1e6 and abs(abs(f - s) - c["Fs_w"]) >= 1e6 for f in EMPTY_OFFSETS for s in c["offsets"])
    return ch


def capture() -> np.ndarray:
    """u8 I,Q of 3 calls x 96 000 samples per channel x R wide samples: as _tuner_capture.rds_capture, plus complex Gaussian
    noise of sigma 0.02 per component (full scale 1) added before the quantisation."""
    c = TC.RDS
    n_wide = CALLS * BYTES_PER_CALL // 2 * c["R"]
    n = np.arange(n_wide, dtype=np.float64)
    rng = np.random.default_rng(SEED)
    zr, zi = NOISE_SIGMA * rng.standard_normal(n_wide), NOISE_SIGMA * rng.standard_normal(n_wide)
    for k, (f_c, a) in enumerate(zip(c["offsets"], c["amplitudes"])):
        x = RG.station_demod(n_wide, if_Fs=c["Fs_w"], pi=c["pi"][k], ps=c["ps"][k], chip_offset=600 * 40 * (1 + 0.3 * k), seed=k + 1)
        phi = np.cumsum(x.astype(np.float64) / (10.0 * c["R"])) + 2 * np.pi * f_c * n / c["Fs_w"]
        zr += a * np.cos(phi)
        zi += a * np.sin(phi)
    iq = np.empty(2 * n_wide, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * zr + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * zi + 0.5), 0, 255)
    return iq
