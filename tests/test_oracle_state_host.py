"""The oracle's state accessors (fmo_pipeline_state_size / _get_state / _set_state, oracle/fm_oracle.c), on the CPU.

The GPU tests compare the device's fmrx_pipeline_get_state / set_state with these, so they are pinned here first, against the
oracle's own data: every serialised vector is compared with the samples the reference defines it by (the last converted input
bytes, the tails of the discriminator output, of the all-pass output and of the mixer output), the size with the formula of
include/fmrx.h, and an oracle resumed from a serialised state with the oracle that simply went on, bit for bit."""
import numpy as np
import pytest

import _pipeline_cases as pc
from _pipeline_cases import same_bits

TAP_SETS = [(101, 101, 101), (13, 13, 13)]
GRID = [(f"mode{m}-{t[0]}", m, {}, t) for m in range(4) for t in TAP_SETS]
OFF_GRID = [(name, pc.CASES[name][0], pc.CASES[name][1], (101, 101, 101)) for name in ("even_stereo_taps", "ratio_3_8")]
ROWS = GRID + OFF_GRID


def _blocks(oracle, p, channels, seed):
    # two blocks to build the state, two more to continue from it; the second is the shortest the stages accept
    n = pc.ragged_blocks(p, channels)
    return pc.stream(oracle, p, [n[0], n[1], n[2], n[1]], seed)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name,mode,edits,taps", ROWS, ids=[r[0] for r in ROWS])
def test_state_vectors_are_the_oracles_data(oracle, name, mode, edits, taps, channels):
    p = pc.oracle_params(oracle, mode, edits, taps)
    Ha, St1, delay, _ = pc.layout(p, channels)
    Tr = p.rf_taps - 1
    po = oracle.pipeline_params(p, channels)
    assert po.state_size() == pc.state_size(p, channels) == len(po.get_state())
    # a fresh handle: project.cpp:61-65, 446-458 (zeros; state_PLL = {0, 0, 1, 0, 1, 0})
    st = po.get_state()
    assert not st[:len(st) - (6 if channels == 2 else 0)].any()
    if channels == 2:
        same_bits(st[-6:], np.array([0, 0, 1, 0, 1, 0], np.float32))
    seen = np.zeros(0, np.uint8)
    for b, blk in enumerate(_blocks(oracle, p, channels, 7 + mode)[:2]):
        out = po.process(blk)
        seen = np.concatenate([seen, blk])
        st = po.get_state()
        f = oracle.u8_to_f32(seen)
        tag = f"{name}, {channels} ch, block {b}"
        same_bits(st[:Tr], f[0::2][-Tr:], "I_state " + tag)
        same_bits(st[Tr:2 * Tr], f[1::2][-Tr:], "Q_state " + tag)
        same_bits(st[2 * Tr:2 * Tr + 2], np.array([out["if_i"][-1], out["if_q"][-1]], np.float32), "prev_i, prev_q " + tag)
        o = 2 * Tr + 2
        demod = out["demod"]
        assert len(demod) >= max(Ha, St1)
        if channels == 1:
            same_bits(st[o:o + Ha], demod[len(demod) - Ha:], "state_mono " + tag)
            assert o + Ha == len(st)
            continue
        same_bits(st[o:o + Ha], po.intermediate("allpass")[-Ha:], "state_mono " + tag)
        o += Ha
        same_bits(st[o:o + St1], demod[-St1:], "state_stereo " + tag)
        same_bits(st[o + St1:o + 2 * St1], demod[-St1:], "state_carrier " + tag)
        o += 2 * St1
        same_bits(st[o:o + Ha], po.intermediate("mixer")[-Ha:], "state_stereofilt " + tag)
        o += Ha
        same_bits(st[o:o + delay], demod[-delay:], "state_allpass " + tag)
        o += delay
        assert o + 6 == len(st)
        assert st[-1] == len(seen) // 2 // p.rf_decim   # trigOffset counts the IF samples of the stream (filter.cpp:37, 62)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name,mode,edits,taps", ROWS, ids=[r[0] for r in ROWS])
def test_resumed_oracle_is_the_oracle_that_went_on(oracle, name, mode, edits, taps, channels):
    p = pc.oracle_params(oracle, mode, edits, taps)
    blocks = _blocks(oracle, p, channels, 21 + mode)
    a = oracle.pipeline_params(p, channels)
    for blk in blocks[:2]:
        a.process(blk)
    st = a.get_state()
    b = oracle.pipeline_params(p, channels)
    b.set_state(st)
    same_bits(b.get_state(), st, "set_state then get_state")
    for k, blk in enumerate(blocks[2:]):
        oa, ob = a.process(blk), b.process(blk)
        tag = f"{name}, {channels} ch, block {k} after the resume"
        assert oa.keys() == ob.keys()
        for key in oa:
            same_bits(oa[key], ob[key], f"{key} {tag}")
        if channels == 2:
            for key in ("carrier_filt", "stereo_filt", "pll", "mixer", "allpass", "mono_filt", "stereo_final"):
                same_bits(a.intermediate(key), b.intermediate(key), f"{key} {tag}")
        same_bits(a.get_state(), b.get_state(), "state " + tag)


def test_wrong_length_is_refused(oracle):
    po = oracle.pipeline(0, 2)
    n = po.state_size()
    assert n == 2 * 100 + 2 + 100 + 2 * 100 + 100 + 50 + 6
    for bad in (n - 1, n + 1, oracle.pipeline(0, 1).state_size()):
        with pytest.raises(ValueError):
            po.set_state(np.zeros(bad, np.float32))
        assert oracle.lib.fmo_pipeline_get_state(po.h, np.zeros(bad, np.float32), bad) == -1
