"""Pipeline parameter sets off the reference's grid, and the block sizes that go with them (test infrastructure only).

The reference ships tap counts {13, 101, 151} and the decimations of its four modes; fmrx_pipeline_create accepts any.  Each
row here edits fields of mode_params(mode, 101, 101, 101) so that a pipeline mixes specialised and parameter-generic stages,
or lands on one of the layout rules of csrc/pipeline.hip (Hd from the band-pass pair, the all-pass delay of an even tap
count, Ha of a rational resampler).  Shared by tests/test_oracle_state_host.py, tests/test_gpu_pipeline_params.py and
tests/test_gpu_pipeline_state.py; the same edits go into the device's Params and the oracle's FmoParams.
"""
from __future__ import annotations

from math import gcd

import numpy as np

# name -> (mode, edits, channel counts the row applies to).  A row whose edit touches only the stereo branch has no mono case:
# its mono pipeline is the shipped one.
CASES = {
    "generic_fe":          (0, dict(rf_taps=64), (1, 2)),
    "generic_fe_decim8":   (0, dict(rf_decim=8, if_Fs=300000, audio_Fs=60000.0), (1, 2)),
    "generic_audio":       (0, dict(audio_taps=51), (1, 2)),
    "generic_audio_dec4":  (0, dict(audio_taps=51, audio_decim=4, audio_Fs=60000.0), (1, 2)),
    "short_bandpass":      (0, dict(stereo_taps=51), (2,)),
    "even_stereo_taps":    (0, dict(stereo_taps=100), (2,)),
    "hd_from_bandpass":    (0, dict(stereo_taps=151, audio_taps=13), (2,)),
    "generic_output":      (0, dict(audio_taps=51, stereo_taps=101), (2,)),
    "all_generic":         (0, dict(rf_taps=64, audio_taps=51, stereo_taps=75), (1, 2)),
    "mode2_short_bandpass": (2, dict(stereo_taps=51), (2,)),
    "ratio_3_8":           (0, dict(audio_upsamp=3, audio_decim=8, audio_taps=303, audio_Fs=90000.0), (1, 2)),
}
# audio_taps is no multiple of audio_upsamp: the reference's state refresh (src/filter.cpp:218-222) and its read (:207) do not
# meet, it is not a stream, and fmrx_pipeline_create refuses the parameters
NOT_A_STREAM = (0, dict(audio_upsamp=3, audio_decim=8, audio_taps=100, audio_Fs=90000.0))

K_RESAMPLE_FRONT = 256   # csrc/fmrx_internal.hpp kResampleFront


def apply_edits(p, edits):
    for k, v in edits.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def oracle_params(oracle, mode, edits, taps=(101, 101, 101)):
    return apply_edits(oracle.mode_params(mode, *taps), edits)


def device_params(fmrx, mode, edits, taps=(101, 101, 101)):
    return apply_edits(fmrx.modeParams(mode, *taps), edits)


def layout(p, channels):
    """(Ha, St-1, delay, Hd) as csrc/pipeline.hip derives them from the parameters."""
    U = p.audio_upsamp
    Ha = (p.audio_taps - 1) // U if U else p.audio_taps - 1
    St1 = p.stereo_taps - 1 if channels == 2 else 0
    delay = St1 // 2
    Hd = Ha + delay
    if channels == 2 and St1 + 3 > Hd:
        Hd = St1 + 3
    if U:
        Hd += K_RESAMPLE_FRONT
    return Ha, St1, delay, (Hd + 3) // 4 * 4 + 4


def state_size(p, channels):
    """The formula of include/fmrx.h (fmrx_pipeline_state_size)."""
    Ha, St1, delay, _ = layout(p, channels)
    n = 2 * (p.rf_taps - 1) + 2 + Ha
    if channels == 2:
        n += 2 * St1 + Ha + delay + 6
    return n


def unit_if(p):
    """IF samples per block unit: audio_decim, or the resampler's period (a block must end on an output boundary)."""
    return p.audio_decim // gcd(p.audio_upsamp, p.audio_decim) if p.audio_upsamp else p.audio_decim


def bytes_of(p, n_if):
    return 2 * p.rf_decim * n_if


def ragged_blocks(p, channels):
    """Four unequal block lengths in IF samples, whole units each: a middling one; the shortest the pipeline accepts (just above
    max(Ha, St-1): below Hd wherever the unit allows, so the next block's history is put together from two buffers); one whose
    byte count is no multiple of 16 where the unit allows (the front end's 16-byte kernels then do not apply); about 3 000."""
    u = unit_if(p)
    Ha, St1, _, Hd = layout(p, channels)
    up = lambda n: -(-n // u) * u
    small = up(max(Ha, St1, 1))
    mid, big = up(1500), up(3000)
    if mid == small:
        mid += u
    cand = [up(2000) + k * u for k in range(16) if up(2000) + k * u not in (mid, small, big)]
    rag = next((c for c in cand if bytes_of(p, c) % 16), cand[0])
    return [mid, small, rag, big]


def resume_blocks(p, n=5):
    """n unequal block lengths of about 2 000 - 3 000 IF samples, whole units, 16-byte multiples (so that every specialised
    kernel is eligible right behind set_state); a resampler whose period is longer than that gets one or two periods."""
    u = unit_if(p)
    while bytes_of(p, u) % 16:
        u *= 2
    if u > 300:   # few units per block: alternate between the two counts nearest the range
        lo = max(1, round(2000 / u))
        hi = max(lo + 1, 3000 // u)
        return [u * k for k in (lo, hi, lo, hi, lo)][:n]
    up = lambda x: -(-x // u) * u
    want = [2000, 2900, 2300, 3000, 2600][:n]
    out = []
    for w in want:
        v = up(w)
        while v in out:
            v += u
        out.append(v)
    return out


def split(iq, p, lengths_if):
    out, off = [], 0
    for n in lengths_if:
        nb = bytes_of(p, n)
        out.append(iq[off:off + nb])
        off += nb
    assert off <= len(iq)
    return out


def stream(oracle, p, lengths_if, seed):
    """The synthetic FM multiplex at the case's input rate, cut into the given blocks."""
    iq = oracle.synth_fm_u8(sum(bytes_of(p, n) for n in lengths_if) // 2, rf_Fs=float(p.rf_Fs), seed=seed)
    return split(iq, p, lengths_if)


def audio_keys(channels):
    return ("audio",) if channels == 1 else ("audio_l", "audio_r")


def same_bits(a, b, msg=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype, msg)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    np.testing.assert_array_equal(a, b, err_msg=msg)
