"""RDS banks (fmrx_rds_bank_*, RdsBank): the RDS chain of N channels per device call.

The bank and the single-stream handle (fmrx_rds) run the same device chain, so every channel is compared with np.array_equal
(no tolerance) against an Rds handle fed the same rows: that pins a channel in any lane to a chain of one channel, and the
device's bit recovery to the host's.  Also: against the stage model (tests/_rds_stage_model.py), against the reference's
model (tests/golden/rds.npz) with the tolerances of test_gpu_rds.py, and behind a receiver bank on the device, against the
oracle (oracle pipeline -> oracle/rds_oracle.py)."""
import os

import numpy as np
import pytest

from _rds_stage_model import stage_model
from _rds_util import BLOCK, N, ROOT, SMALL, bank_streams, ht, rds_iq_u8, rel, same

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "rds.npz"))
TAPS = ("channel", "carrier", "pll_i", "pll_q", "resampled_i", "pll_state")


@pytest.mark.parametrize("mode", [0, 2])
def test_bank_equals_single_stream_handles(fmrx, mode):
    """Both sides run the same kernels, so this proves two things, bit for bit: channel c of a 70-channel bank (a lane other
    than 0, the second wave only partly filled) equals a chain of one channel; and the device's clock and data recovery
    (rdsb_cdr_kernel, which only the bank runs) equals the host's cdr(), which the single-stream handle calls."""
    nb = 6
    rows = bank_streams(nb)
    bank = fmrx.RdsBank(mode, N, BLOCK)
    singles = [fmrx.Rds(mode, max_block=BLOCK) for _ in range(N)]
    synced = 0
    for b in range(nb):
        blk = rows[:, b * BLOCK:(b + 1) * BLOCK]
        got = bank.process(blk)
        for c in range(N):
            want = singles[c].process(blk[c])
            for k in ("rrc_i", "rrc_q", "diff_bits"):
                same(got[k][c], want[k], f"mode {mode} block {b} channel {c}: {k}")
            assert got["offset_type"][c] == want["offset_type"], (mode, b, c)
            synced += want["offset_type"] != " "
            if c in (0, 9, 63, 64, 69):
                for tap in TAPS:
                    same(bank.read_tap(c, tap), singles[c].read_tap(tap), f"mode {mode} block {b} channel {c}: tap {tap}")
    assert synced > N, "the fixture must exercise frame synchronisation"
    bank.close()


def test_bank_remainder_paths_in_every_lane(fmrx):
    """A block of 333 samples (no rate change) leaves 13 samples to the PLL lanes' remainder loop and one to the FIR's last
    quad: 70 channels over three blocks against 70 single-stream handles, bit for bit."""
    n, nb = 333, 3
    rows = bank_streams(nb, block=n)
    p = fmrx.RdsParams(*SMALL)
    bank = fmrx.RdsBank(params=p, n_channels=N, block=n)
    singles = [fmrx.Rds(params=p, max_block=n) for _ in range(N)]
    for b in range(nb):
        blk = rows[:, b * n:(b + 1) * n]
        got = bank.process(blk)
        for c in range(N):
            want = singles[c].process(blk[c])
            for k in ("rrc_i", "rrc_q", "diff_bits"):
                same(got[k][c], want[k], f"block {b} channel {c}: {k}")
            assert got["offset_type"][c] == want["offset_type"], (b, c)
            if c in (0, 9, 63, 64, 69):
                for tap in TAPS:
                    same(bank.read_tap(c, tap), singles[c].read_tap(tap), f"block {b} channel {c}: tap {tap}")
    bank.close()


def test_bank_stages_equal_the_stage_model(fmrx):
    """Channels 0, 63 and 69 of 70 (the first and last lane of a full wave, the last of a partial one) at block 333 against
    tests/_rds_stage_model.py, bit for bit, over two blocks (the second runs on carried histories)."""
    n, nb = 333, 2
    rows = bank_streams(nb, block=n)
    p = fmrx.RdsParams(*SMALL)
    bank = fmrx.RdsBank(params=p, n_channels=N, block=n)
    models = {c: stage_model(fmrx, p) for c in (0, 63, 69)}
    for b in range(nb):
        blk = rows[:, b * n:(b + 1) * n]
        got = bank.process(blk)
        for c, m in models.items():
            dev = {k: bank.read_tap(c, k) for k in TAPS}
            dev.update(rrc_i=got["rrc_i"][c], rrc_q=got["rrc_q"][c])
            for k, want in m.step(blk[c], dev).items():
                same(dev[k], want, f"block {b} channel {c}: {k}")
            assert dev["pll_state"][5] == (b + 1) * n
    bank.close()


def test_bank_against_the_reference_model(fmrx):
    x = G["fm_demod"]
    rows = bank_streams(4)
    rows[0], rows[N - 1] = x[:4 * BLOCK], x[:4 * BLOCK]
    bank = fmrx.RdsBank(0, N, BLOCK)
    for b in range(4):
        out = bank.process(rows[:, b * BLOCK:(b + 1) * BLOCK])
        for c in (0, N - 1):
            for k in ("channel", "carrier", "pll_i", "pll_q", "resampled_i"):
                e = rel(ht(bank.read_tap(c, k)), G[f"b{b}_{k}_ht"])
                assert e <= 1e-9, (b, c, k, e)
            for k in ("rrc_i", "rrc_q"):
                e = rel(out[k][c], G[f"b{b}_{k}"])
                assert e <= 1e-9, (b, c, k, e)
            np.testing.assert_array_equal(out["diff_bits"][c], G[f"b{b}_diff_bits"].astype(np.uint8))
            fs = G[f"b{b}_framesync"]
            assert (ord(out["offset_type"][c][0]), len(out["offset_type"][c])) == (int(fs[0]), int(fs[1])), (b, c, out["offset_type"][c])
    for c in (0, N - 1):
        assert rel(bank.read_tap(c, "pll_state"), G["pll_state"]) <= 1e-9


def test_bank_reset(fmrx):
    rows = bank_streams(4)
    bank = fmrx.RdsBank(0, N, BLOCK)
    cont = [fmrx.Rds(0, max_block=BLOCK) for _ in range(N)]
    fresh = fmrx.Rds(0, max_block=BLOCK)
    blocks = [rows[:, b * BLOCK:(b + 1) * BLOCK] for b in range(4)]
    for b in range(2):
        bank.process(blocks[b])
        for c in range(N):
            cont[c].process(blocks[b][c])
    bank.reset(9)                                         # one channel, mid-stream: it starts over, the others go on
    for b in range(2, 4):
        got = bank.process(blocks[b])
        for c in range(N):
            want = fresh.process(blocks[b][c]) if c == 9 else cont[c].process(blocks[b][c])
            for k in ("rrc_i", "rrc_q", "diff_bits"):
                same(got[k][c], want[k], f"block {b} channel {c}: {k}")
            assert got["offset_type"][c] == want["offset_type"], (b, c)
    bank.reset()                                          # all channels = a fresh bank
    other = fmrx.RdsBank(0, N, BLOCK)
    for b in range(2):
        got, want = bank.process(blocks[b + 2]), other.process(blocks[b + 2])
        for c in range(N):
            for k in ("rrc_i", "rrc_q", "diff_bits"):
                same(got[k][c], want[k][c], f"after reset(-1): block {b} channel {c}: {k}")
            assert got["offset_type"][c] == want["offset_type"][c]


def _receiver_to_rds(fmrx, ch, rds_mode, iqs, n_blocks):
    """Blocks through a receiver bank on the device, then its discriminator rows through an RDS bank on the same stream;
    compared with an RDS bank fed the same rows from the host."""
    import torch
    n = len(iqs)
    stream = torch.cuda.Stream()
    d_iq = torch.from_numpy(np.stack(iqs)).cuda()
    audio = torch.zeros(n * ch.audio_channels * ch.n_audio, dtype=torch.float32, device="cuda")
    pcm = torch.zeros(n * ch.audio_channels * ch.n_audio, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ptr, pitch, n_if = ch.demod_layout()
    assert n_if == BLOCK
    dev, host = fmrx.RdsBank(rds_mode, n, n_if), fmrx.RdsBank(rds_mode, n, n_if)
    outs = []
    for b in range(n_blocks):
        blk = d_iq[:, b * 192000:(b + 1) * 192000].contiguous()
        torch.cuda.synchronize()
        ch.load_dev(blk.data_ptr(), stream=stream.cuda_stream)
        ch.process_dev(audio.data_ptr(), pcm.data_ptr(), stream=stream.cuda_stream)
        dev.process_dev(ptr, pitch, stream=stream.cuda_stream)
        got = dev.collect()
        rows = np.stack([ch.read_tap(c, "demod") for c in range(n)])
        want = host.process(rows)
        for c in range(n):
            for k in ("rrc_i", "rrc_q", "diff_bits"):
                same(got[k][c], want[k][c], f"block {b} channel {c}: {k}")
            assert got["offset_type"][c] == want["offset_type"][c]
        outs.append(got)
    return outs


def test_receiver_bank_to_rds_bank_on_the_device(fmrx, oracle):
    import rds_oracle as R
    nb, n = 4, 3
    fixtures = [rds_iq_u8(nb, seed=5 + c, chip_offset=600.0 + 97 * c) for c in range(n)]
    iqs = [f[0] for f in fixtures]
    # the exact stereo bank: its discriminator rows equal the oracle's bit for bit, so bits and offsets equal the oracle's chain
    ch = fmrx.Channels(0, n, audio_channels=2, exact=True, block_bytes=192000)
    outs = _receiver_to_rds(fmrx, ch, 0, iqs, nb)
    for c in range(n):
        pl, chain = oracle.pipeline(0, 2), R.RdsChain()
        synced = 0
        for b in range(nb):
            want = chain.process(pl.process(iqs[c][b * 192000:(b + 1) * 192000])["demod"])
            np.testing.assert_array_equal(outs[b]["diff_bits"][c], want["diff_bits"].astype(np.uint8), err_msg=f"channel {c} block {b}")
            assert outs[b]["offset_type"][c] == want["offset_type"], (c, b)
            synced += want["offset_type"] != " "
        assert synced >= 2, c
    ch.close()
    # the fast stereo bank, and the mono bank of mode 2: against the host-row path
    ch = fmrx.Channels(0, n, audio_channels=2, exact=False, block_bytes=192000)
    _receiver_to_rds(fmrx, ch, 0, iqs, 2)
    ch.close()
    ch = fmrx.Channels(2, n, audio_channels=1, exact=False, block_bytes=192000)
    _receiver_to_rds(fmrx, ch, 2, iqs, 2)
    ch.close()


def test_bank_refusals(fmrx):
    with pytest.raises(fmrx.FmrxError):
        fmrx.RdsBank(0, 4, block=9601)                    # block*upsamp not a multiple of decim
    p = fmrx.RdsParams(240000, 151, 1, 1, 26, 101)
    with pytest.raises(fmrx.FmrxError):
        fmrx.RdsBank(n_channels=4, block=100, params=p)    # shorter than the band-pass histories
    with pytest.raises(fmrx.FmrxError):
        fmrx.RdsBank(1, 4)                                # the model defines no RDS rates for mode 1
    bank = fmrx.RdsBank(0, N, BLOCK)
    for bad in (N, N + 5):
        with pytest.raises(fmrx.FmrxError):
            bank.reset(bad)
    for bad in (-1, N):
        with pytest.raises(fmrx.FmrxError):
            bank.read_tap(bad, "rrc_i")
    import torch
    d = torch.zeros(N * BLOCK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(fmrx.FmrxError):
        bank.collect()                                    # nothing to collect
    bank.process_dev(d.data_ptr(), BLOCK)
    with pytest.raises(fmrx.FmrxError):
        bank.process_dev(d.data_ptr(), BLOCK)             # the previous call's bits are not collected yet
    with pytest.raises(fmrx.FmrxError):
        bank.reset()
    out = bank.collect()
    assert len(out["diff_bits"]) == N
    bank.process_dev(d.data_ptr(), BLOCK)                 # collected: the next call goes through
    bank.collect()
    mono = fmrx.Channels(0, 2)
    with pytest.raises(fmrx.FmrxError):
        mono.demod_layout()                               # the fused mono bank keeps no discriminator rows
