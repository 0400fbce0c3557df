"""The RDS path on the GPU (float64 HIP kernels + host bit recovery, fmrx_rds_*) against the golden vectors of the reference's
own Python model (tests/golden/rds.npz: model/fmSupportLib.py imported in the build container) and against the numpy oracle
(oracle/rds_oracle.py, pinned to the same vectors) on a second, noisy stream.

Tolerances: every signal stage is float64 on both sides; the FIRs sum in the model's order, sin / cos / atan2 are the
device's double-precision functions against glibc's (last-bit differences that the loop carries along): 1e-9 of full
scale on the matched-filter output over four blocks (measured ~1e-13), bits and frame-sync results identical.

The handle runs the RDS bank's device chain with one channel (csrc/rds_chain.hpp).  The stages that only multiply and add are
also checked bit for bit against tests/_rds_stage_model.py, on small blocks of changing size that reach the kernels' remainder
paths; the same blocks against the oracle to 1e-8 (measured: <= 2e-12, the PLL row; the other rows <= 4e-13)."""
import os

import numpy as np
import pytest

from _rds_stage_model import stage_model
from _rds_util import ROOT, SMALL, ht, rel, same

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "rds.npz"))
# small and varying blocks, none of them the largest first: mode 0 (blocks are multiples of 960), and a chain without rate
# change whose blocks leave 13, 14, 15, 12 samples to the PLL lanes' remainder loop and 1, 2, 3, 0 to the FIR's last quad
SEQUENCES = [(None, 2880, (960, 2880, 960, 1920)), (SMALL, 333, (333, 270, 303, 332))]


def small_stream():
    from rds_signal import rds_demod_signal
    return rds_demod_signal(9600, 240e3, seed=21, chip_offset=66.0, noise=0.01)[0]


def make_rds(fmrx, params, max_block):
    return fmrx.Rds(0, max_block=max_block, params=fmrx.RdsParams(*params) if params else None)


def test_rds_chain_against_the_reference_model(fmrx):
    r = fmrx.Rds(0)
    x, n = G["fm_demod"], 9600
    worst = 0.0
    for b in range(4):
        out = r.process(x[b * n:(b + 1) * n])
        for k in ("channel", "carrier", "pll_i", "pll_q", "resampled_i"):
            e = rel(ht(r.read_tap(k)), G[f"b{b}_{k}_ht"])
            assert e <= 1e-9, (b, k, e)
            worst = max(worst, e)
        for k in ("rrc_i", "rrc_q"):
            e = rel(out[k], G[f"b{b}_{k}"])
            assert e <= 1e-9, (b, k, e)
            worst = max(worst, e)
        np.testing.assert_array_equal(out["diff_bits"], G[f"b{b}_diff_bits"].astype(np.uint8))
        fs = G[f"b{b}_framesync"]
        assert (ord(out["offset_type"][0]), len(out["offset_type"])) == (int(fs[0]), int(fs[1])), (b, out["offset_type"])
    assert rel(r.read_tap("pll_state"), G["pll_state"]) <= 1e-9
    print("largest relative deviation from the model over 4 blocks:", worst)
    # sanity of the fixture itself: within a block the recovered bits ARE the transmitted ones (differential coding removes the
    # phase ambiguity of the recovered carrier; the first bit of a block has no predecessor: the model re-makes its CDR state
    # every block, model/fmMonoBlock.py:276-280)
    tx = G["tx_bits"]
    for b in range(4):
        got = G[f"b{b}_diff_bits"].astype(np.uint8)[1:]
        assert max(np.mean(got == tx[s:s + len(got)]) for s in range(250)) >= 0.97, b


def test_rds_chain_noisy_stream_against_the_oracle(fmrx):
    import rds_oracle as R
    from rds_signal import rds_demod_signal
    x, _ = rds_demod_signal(6 * 9600, 240e3, seed=21, chip_offset=66.0, noise=0.01)
    r, o = fmrx.Rds(0), R.RdsChain()
    for b in range(6):
        blk = x[b * 9600:(b + 1) * 9600]
        got, want = r.process(blk), o.process(blk)
        assert rel(got["rrc_i"], want["rrc_i"]) <= 1e-8 and rel(got["rrc_q"], want["rrc_q"]) <= 1e-8
        np.testing.assert_array_equal(got["diff_bits"], want["diff_bits"].astype(np.uint8))
        assert got["offset_type"] == want["offset_type"]
    r.reset()
    got = r.process(x[:9600])
    o2 = R.RdsChain()
    assert rel(got["rrc_i"], o2.process(x[:9600])["rrc_i"]) <= 1e-9
    with pytest.raises(fmrx.FmrxError):
        r.process(x[:9601])                      # n*upsamp not a multiple of decim
    with pytest.raises(fmrx.FmrxError):
        fmrx.Rds(1)                              # the model defines no RDS rates for mode 1


@pytest.mark.parametrize("params,max_block,blocks", SEQUENCES, ids=["mode0", "no_rate_change"])
def test_rds_stages_equal_the_stage_model(fmrx, params, max_block, blocks):
    """Every multiply-add stage of the chain equals tests/_rds_stage_model.py bit for bit (the model is fed the device's own
    taps of the stage before), and the PLL rows and state are carried from block to block as the layout says."""
    x = small_stream()
    r = make_rds(fmrx, params, max_block)
    m = stage_model(fmrx, r.params)
    at, prev = 0, None
    for n in blocks:
        out = r.process(x[at:at + n])
        dev = {k: r.read_tap(k) for k in ("channel", "carrier", "pll_i", "pll_q", "resampled_i", "pll_state")}
        dev.update(rrc_i=out["rrc_i"], rrc_q=out["rrc_q"])
        for k, want in m.step(x[at:at + n], dev).items():
            same(dev[k], want, f"block at {at} of {n}: {k}")
        assert len(dev["pll_i"]) == len(dev["pll_q"]) == n + 1
        for k in ("pll_i", "pll_q"):                 # [0] = the block before's last; the start state has 1.0 for both (fmMonoBlock.py:186)
            same(dev[k][:1], prev[k][-1:] if prev else np.array([1.0]), f"block at {at}: {k}[0]")
        same(dev["pll_state"][[4, 6]], np.array([dev["pll_i"][n], dev["pll_q"][n]]), f"block at {at}: the state's NCO pair")
        at += n
        assert dev["pll_state"][5] == at
        prev = dev


@pytest.mark.parametrize("params,max_block,blocks", SEQUENCES, ids=["mode0", "no_rate_change"])
def test_rds_small_and_varying_blocks_against_the_oracle(fmrx, params, max_block, blocks):
    """Blocks far smaller than 9600 and of changing size against oracle/rds_oracle.py, with the bound of
    test_rds_chain_noisy_stream_against_the_oracle (1e-8 of full scale) on the matched-filter rows and the taps; bits and
    frame-sync results equal.  Every block yields at least one bit and finite rows."""
    import rds_oracle as R
    x = small_stream()
    r = make_rds(fmrx, params, max_block)
    p = r.params
    o = R.RdsChain(p.if_Fs, p.taps, p.upsamp, p.decim, p.sps, p.rrc_taps)
    at = 0
    for n in blocks:
        got, want = r.process(x[at:at + n]), o.process(x[at:at + n])
        assert len(want["diff_bits"]) >= 1 and np.isfinite(got["rrc_i"]).all() and np.isfinite(got["rrc_q"]).all(), (at, n)
        for k in ("rrc_i", "rrc_q", "channel", "carrier", "pll_i", "resampled_i"):
            e = rel(got[k] if k in got else r.read_tap(k), want[k])
            print(f"block at {at} of {n}: {k} {e:.3e}")
            assert e <= 1e-8, (at, n, k, e)
        np.testing.assert_array_equal(got["diff_bits"], want["diff_bits"].astype(np.uint8))
        assert got["offset_type"] == want["offset_type"]
        at += n


def test_rds_process_dev_then_process(fmrx):
    """process_dev recovers no bits and does not count a block: two of them in a row are legal, the tap counts are the second
    call's, and the process that follows reports its block's bits in the CDR's block_count == 0 form.  A fresh handle fed the
    same three blocks through process has the same rows and taps; its third block's bits are the block_count != 0 form (one
    more bit in front for every re-start of the recovery, fmSupportLib.py:103-200; the stream is placed so that there is one)."""
    import torch
    from rds_signal import rds_demod_signal
    x = rds_demod_signal(9600, 240e3, seed=21, chip_offset=80.0, noise=0.01)[0]
    blocks = (960, 1920, 1920)
    a, b = fmrx.Rds(0, max_block=2880), fmrx.Rds(0, max_block=2880)
    for k in ("channel", "pll_i", "pll_q", "rrc_i"):
        assert len(a.read_tap(k)) == 0, k            # nothing has run: no samples, the PLL rows included
    assert len(a.read_tap("pll_state")) == 7
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    at = 0
    for n in blocks[:2]:
        a.process_dev(d[at:at + n].data_ptr(), n)
        want = b.process(x[at:at + n])
        at += n
    assert (len(a.read_tap("channel")), len(a.read_tap("pll_i")), len(a.read_tap("pll_q"))) == (1920, 1921, 1921)
    assert len(a.read_tap("resampled_i")) == len(a.read_tap("rrc_i")) == len(a.read_tap("rrc_q")) == 1920 * 247 // 960
    same(a.read_tap("rrc_i"), want["rrc_i"], "rrc_i after two process_dev calls")
    got, want = a.process(x[at:at + blocks[2]]), b.process(x[at:at + blocks[2]])
    for k in ("rrc_i", "rrc_q"):
        same(got[k], want[k], k)
    for k in ("channel", "carrier", "pll_i", "pll_q", "resampled_i", "pll_state"):
        same(a.read_tap(k), b.read_tap(k), k)
    # the host primitives on the same row: block_count 0 is what the handle without a counted block reports
    forms = []
    for count in (0, 2):
        bits, _ = fmrx.CDR(got["rrc_i"], a.params.sps, [np.zeros(2), 158, 0], count)
        forms.append(fmrx.diff_decoding(bits).astype(np.uint8))
    assert len(forms[0]) != len(forms[1]), "the fixture must tell the two forms apart"
    np.testing.assert_array_equal(got["diff_bits"], forms[0])
    np.testing.assert_array_equal(want["diff_bits"], forms[1])
