"""mono_fused_kernel's straight-line schedule (kernels_fe_mfma.hip), bit for bit against the fma-chain model of
tests/_fir_model.py, with the run edges placed at every position the schedule distinguishes.

Tile t of a wave's run sits in ring slot t mod NSLOT, and a straight-line batch (TB tiles) is compiled once per start
slot: in mode 0 (TB 10, NSLOT 4) a batch starts on slot 0 or 2, in mode 1 (TB 12, NSLOT 6) always on slot 0.  A wave owns
ceil(batches / 2048) consecutive batches (2048 waves in the largest grid), so the block sizes below give runs of one,
two and three batches: with one or three, neighbouring waves start on different slots; with two, every run starts on
slot 0 and ends on slot 2.  Sizes that are not a whole number of batches leave the last wave a partial run (t_fast1 and
fast_last fall elsewhere) and an odd number of tiles.  A call's first block is carried into the next, so the later
blocks also start with a dry tile in front of every run but the first."""
import numpy as np
import pytest

from test_gpu_channels import channel_stream
from test_gpu_fir_exact import taps_of
from test_gpu_mfma_exact import FUSED_CASES, MODE_OF_DECIM, check_fused, run_fused

pytestmark = pytest.mark.gpu

WAVES = 2048   # waves of the largest fused grid (256 CUs x 2 workgroups x 4 waves)


def schedule_blocks(runs):
    """Audio outputs per block (multiples of 4: 16-byte aligned blocks) for the given batches per wave: every wave but
    the last owns whole batches, the last one ends in a partial batch (an odd number of tiles)."""
    return [256 * 7 if r == 1 else 256 * (WAVES * (r - 1) + 3) + 132 for r in runs]


@pytest.mark.parametrize("T,D,TA,DA", FUSED_CASES)
def test_fused_schedule_short_runs(fmrx, oracle, T, D, TA, DA):
    """Every fused shape: runs of one batch on either start slot (7 and 10 waves, the last run of the second block
    partial), then a carried block of 4 batches."""
    mode = MODE_OF_DECIM[DA]
    p = fmrx.modeParams(mode, T, TA)
    cuts = [2 * D * DA * n for n in schedule_blocks([1]) + [256 * 9 + 4, 256 * 3 + 8]]
    iq = channel_stream(oracle, 5, sum(cuts) // 2, p.rf_Fs)
    blocks, o = [], 0
    for c in cuts:
        blocks.append(iq[o:o + c])
        o += c
    res = run_fused(fmrx, mode, T, TA, blocks, wraps=(True,))
    check_fused(oracle, res, taps_of(fmrx, p)[2], T, D, TA, DA, f"fused {T}/{D}/{TA}/{DA} short runs", True)


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_schedule_long_runs(fmrx, oracle, mode):
    """The bench shape of each mode: runs of two batches per wave (all starting on slot 0), then of three (the first
    batch on both start slots, t_fast1 and fast_last on either); the last wave's run ends in a partial batch."""
    p = fmrx.modeParams(mode)
    D, DA = p.rf_decim, p.audio_decim
    cuts = [2 * D * DA * n for n in schedule_blocks([2, 3])]
    iq = channel_stream(oracle, 7, sum(cuts) // 2, p.rf_Fs)
    blocks, o = [], 0
    for c in cuts:
        blocks.append(iq[o:o + c])
        o += c
    res = run_fused(fmrx, mode, p.rf_taps, p.audio_taps, blocks, wraps=(True,))
    check_fused(oracle, res, taps_of(fmrx, p)[2], p.rf_taps, D, p.audio_taps, DA, f"fused mode {mode} long runs", True)
    n_batches = [-(-len(r["audio"]) // 256) for r in res]
    assert [-(-n // WAVES) for n in n_batches] == [2, 3]
