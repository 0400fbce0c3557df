"""meters_mpx_kernel bit for bit against the order of its additions (tests/_meters_order_model.py), at row lengths of several
batches of 16 segments.  The kernel promises "float64 in a FIXED order"; tests/test_gpu_meters.py allows it 1e-10 of a sum's
scale at 1, 2 and 9 segments.  Here every float64 of the MPX group is compared as bits (any NaN equal to any NaN), the model
runs on the CPU with the library's own table, and tests/test_meters_order_model_host.py shows that six mistakes in the order --
an unfused multiply-add, the wave butterfly run upwards, the waves added in pairs, the segments' powers added in another order, a
stale LDS buffer, the tail taken first -- each change these bits on these rows (tests/_meters_exact_cases.py).

Rows are uniform in +-1.5 from fixed seeds and sit on the device at a pitch of n_if + 5 floats; every gap and the space behind
the last row hold NaN, so a load past a row's end poisons a sum.  A row whose address is a multiple of 16 takes one 16-byte load
per thread and segment, any other row four 4-byte loads.  What each case reaches:

| case                      | segments M | look-ahead at its start        | batches of 16: full + rest | LDS buffer 0 written again   | channels per workgroup | tail samples  | loads               |
|---------------------------|------------|--------------------------------|----------------------------|------------------------------|------------------------|---------------|---------------------|
| a: 1 / 2 / 3              | 1 / 2 / 3  | no load ahead / one / both     | 0 + 1 / 0 + 2 / 0 + 3      | no                           | 1                      | 1023 / 0 / 1  | both, see below     |
| a: 15 / 16 / 17           | as named   | full depth                     | 0 + 15 / 1 + 0 / 1 + 1     | no                           | 1                      | 255, 256, 257 | both, see below     |
| a: 31 / 32 / 33           | as named   | full depth                     | 1 + 15 / 2 + 0 / 2 + 1     | no / no / by batch 2         | 1                      | 1023 / 0 / 1  | both, see below     |
| a: 49 / 75                | as named   | full depth                     | 3 + 1 / 4 + 11             | by batch 2 / by batches 2, 4 | 1                      | 257 / 0       | both, see below     |
| b: 17 x 1024 + 3          | 17         | full depth, again per channel  | 1 + 1                      | no                           | 2 or 3, unlike rows    | 3             | 16-byte alone       |
| b: 33 x 1024              | 33         | full depth, again per channel  | 2 + 1                      | by batch 2, then by the next channel's batch 0 | 2 or 3, unlike rows | 0 | both (the pitch is odd) |
| c: 17 x 1024 + 7          | 17         | full depth                     | 1 + 1                      | no                           | 1                      | 7             | both, see below     |
| c: 33 x 1024 + 7          | 33         | full depth                     | 2 + 1                      | by batch 2                   | 1                      | 7             | both, see below     |
| d: a bank call, 8 blocks  | 75         | full depth                     | 4 + 11                     | by batches 2, 4              | 1                      | 0             | the bank's layout   |
| d: 259 samples short      | 74         | full depth                     | 4 + 10                     | by batches 2, 4              | 1                      | 765           | the bank's layout   |

(b)'s first length has a pitch of 17 416 floats, a multiple of 4: every row takes the 16-byte load.  Every case of (a) and (c) runs twice: from a 16-byte aligned base and from one float past it.  With the pitch n_if + 5 and
rows 0, 1, 2 that is, by tail mod 4: tail 0 (pitch = 1 mod 4): rows (16 B, 4 B, 4 B), then (4 B, 4 B, 16 B); tail 1 (pitch = 2):
(16, 4, 16), then all 4 B; tails 255, 1023 and 7 (pitch = 0): all 16 B, then all 4 B; tail 256 (pitch = 1) as tail 0; tail 257
(pitch = 2) as tail 1.  The result must not depend on it: both runs are compared with the same model record.

Nothing of a reference tree is read; the CPU side is numpy alone."""
import numpy as np
import pytest

import _meters_exact_cases as mc
import _meters_model as mm
import _meters_order_model as om

pytestmark = pytest.mark.gpu

IF_FS, L = mc.IF_FS, mm.SEGMENT
MPX_BLOCKS_PER_CU = 3      # kMpxBlocksPerCu of csrc/meters.hip: the MPX pass's grid is capped at this many workgroups per CU


@pytest.fixture(scope="module")
def table(fmrx):
    return fmrx.metersTable(IF_FS)


_models = {}


def models(key, rows, table):
    """the order model's records of `rows`, computed once per key"""
    if key not in _models:
        _models[key] = mc.model(rows, table)
    return _models[key]


def on_device(torch, rows, base):
    """rows [N][n] -> a device tensor of NaN with the rows at `base` floats from its 16-byte aligned start and a pitch of
    n + 5; returns (tensor, address of row 0, pitch)"""
    N, n = rows.shape
    pitch = n + mc.PITCH_EXTRA
    buf = np.full(base + N * pitch, np.nan, np.float32)
    buf[base:].reshape(N, pitch)[:, :n] = rows
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * base, pitch


def run_mpx(fmrx, n_channels, ptr, pitch, n_if):
    m = fmrx.Meters(IF_FS, n_channels)
    m.process_dev(None, 0, 0, ptr, pitch, n_if)
    got = m.collect()
    m.close()
    return got


def check_bits(got, want, n_if, what):
    """got: METER_DTYPE [N]; want: [N] dicts of the model"""
    assert len(got) == len(want)
    for c, w in enumerate(want):
        assert got["n_if"][c] == n_if and got["segments"][c] == n_if // L, f"{what}: channel {c}: counts"
        bad = mc.differing_fields(got[c], w)
        assert not bad, (f"{what}: channel {c}: {', '.join(bad)} differ from the order model: "
                         + "; ".join(f"{f} {got[c][f]!r} for {w[f]!r}" for f in om.FIELDS))


@pytest.mark.parametrize("M,tail", mc.A_CASES, ids=lambda v: str(v))
def test_a_row_lengths(fmrx, table, M, tail):
    import torch
    rows = mc.a_rows(M, tail)
    n_if = M * L + tail
    assert rows.shape == (2 if M >= 49 else 3, n_if)
    want = models(("a", M, tail), rows, table)
    for base in (0, 1):
        t, ptr, pitch = on_device(torch, rows, base)
        got = run_mpx(fmrx, len(rows), ptr, pitch, n_if)
        check_bits(got, want, n_if, f"M = {M}, tail {tail}, base {base}")
    if M >= 2:
        # the equality above is not one that any way of adding would meet: the definition's plain sums have other bits
        plain = [mm.mpx_group(r, IF_FS)["probe"] for r in rows]
        assert any((np.asarray(w["probe"]).view(np.uint64) != p.view(np.uint64)).any() for w, p in zip(want, plain))
        assert any((got["probe"][c].view(np.uint64) != p.view(np.uint64)).any() for c, p in enumerate(plain))


@pytest.mark.parametrize("n_if", mc.B_LENGTHS)
def test_b_one_workgroup_walks_several_channels(fmrx, table, n_if):
    """8 x CUs + 5 channels over a grid of 3 x CUs workgroups: each walks two or three channels, `cap` apart, whose rows differ
    (channels cycle over nb base rows and cap is no multiple of nb) and one of which holds a NaN in its second batch.  At 33
    segments a channel's last batch sits in LDS buffer 0, where the next channel's first batch goes."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = MPX_BLOCKS_PER_CU * cus
    nb = mc.b_base(cap)
    N = 8 * cus + 5
    assert cap % nb != 0 and N > 2 * cap and n_if // L > 16
    base = mc.b_rows(nb, n_if)
    assert np.isnan(base[mc.B_NAN_ROW, 16 * L:32 * L]).any() and np.isfinite(np.delete(base, mc.B_NAN_ROW, 0)).all()
    want = models(("b", nb, n_if), base, table)
    pitch = n_if + mc.PITCH_EXTRA
    padded = torch.full((nb, pitch), float("nan"), dtype=torch.float32, device="cuda")
    padded[:, :n_if] = torch.from_numpy(base.copy()).cuda()
    idx = torch.arange(N, device="cuda") % nb
    rows = padded[idx]                                           # [N][pitch], built on the device; the gaps are NaN
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 0
    got = run_mpx(fmrx, N, rows.data_ptr(), pitch, n_if)
    assert np.all(got["n_if"] == n_if) and np.all(got["segments"] == n_if // L)
    got_bits = np.stack([om.bits(got[c]) for c in range(N)])
    want_bits = np.stack([om.bits(w) for w in want])[np.arange(N) % nb]
    bad = np.flatnonzero((got_bits != want_bits).any(axis=1))
    assert len(bad) == 0, (f"{len(bad)} of {N} channels differ from the model of their base row, the first {bad[:8]} "
                           f"(workgroups {bad[:8] % cap}, base rows {bad[:8] % nb}): fields "
                           f"{mc.differing_fields(got[bad[0]], want[bad[0] % nb])}")
    # and, NaNs included, the same row gives the same bytes wherever a workgroup meets it
    mpx = np.stack([got[f] for f in ("sum_x", "sum_x2", "max_abs")] + [got["probe"][:, p] for p in range(8)], axis=1).view(np.uint64)
    assert np.array_equal(mpx, mpx[np.arange(N) % nb])


@pytest.mark.parametrize("n_if", mc.C_LENGTHS)
def test_c_special_values(fmrx, table, n_if):
    import torch
    rows = mc.c_rows(n_if)
    M = n_if // L
    assert rows.shape == (4, n_if)
    assert np.flatnonzero(np.isnan(rows[0])).tolist() == [3 * L + 802]
    assert np.flatnonzero(np.isinf(rows[1])).tolist() == [16 * L + 517, M * L + 2] and rows[1, 16 * L + 517] > 0 > rows[1, M * L + 2]
    assert np.isfinite(rows[2:]).all() and np.signbit(rows[2][rows[2] == 0]).any() and np.abs(rows[2]).max() > 2.9e38
    assert ((rows[2] != 0) & (np.abs(rows[2]) < np.finfo(np.float32).tiny)).any()
    want = models(("c", n_if), rows, table)
    for base in (0, 1):
        t, ptr, pitch = on_device(torch, rows, base)
        got = run_mpx(fmrx, 4, ptr, pitch, n_if)
        check_bits(got, want, n_if, f"n_if {n_if}, base {base}")
        assert np.isfinite(got["max_abs"][0]) and got["max_abs"][0] == float(np.nanmax(np.abs(rows[0])))
        assert np.isnan(got["sum_x"][0]) and np.isnan(got["probe"][0][:5]).all()
        assert got["max_abs"][1] == np.inf
        # the ordinary row beside them reads what it reads alone
        alone = run_mpx(fmrx, 1, ptr + 4 * 3 * pitch, pitch, n_if)
        assert alone[0].tobytes() == got[3].tobytes()
        assert np.isfinite(om.bits(got[3]).view(np.float64)).all()


ROBUST_MUTANTS = tuple(m for m in om.MUTANTS if m != "tail_first")


def test_d_behind_a_bank_call_of_8_reference_blocks(fmrx, table):
    """5 synthetic stereo stations -> a fast stereo bank of mode 0 whose call is 8 x 192 000 bytes -> Meters.for_bank on the
    bank's own layouts: 76 800 discriminator samples per channel, 75 segments, five batches."""
    import torch
    N, bb = mc.D_CHANNELS, mc.D_BLOCK_BYTES
    iq = mc.d_streams()
    bank = fmrx.Channels(0, N, audio_channels=2, block_bytes=bb)
    assert float(bank.params.if_Fs) == IF_FS
    meters = fmrx.Meters.for_bank(bank)
    d_iq = torch.from_numpy(iq.copy()).cuda()
    d_audio = torch.zeros((N, 2, bank.n_audio), dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros((N, bank.n_audio, 2), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    bank.load_dev(d_iq.data_ptr(), stream=s)
    bank.process_dev(d_audio.data_ptr(), d_pcm.data_ptr(), stream=s)
    meters.process_bank(stream=s)
    got = meters.collect()
    stream.synchronize()
    rows = np.stack([bank.read_tap(c, "demod") for c in range(N)])
    n_if = rows.shape[1]
    assert n_if == 75 * L == bank.demod_layout()[2] and np.isfinite(rows).all()
    want = models(("d", n_if), rows, table)
    check_bits(got, want, n_if, "bank call")
    for c in range(N):
        rf = mm.rf_group(iq[c])
        for f in mm.RF_FIELDS:
            assert got[f][c] == rf[f], f"channel {c}: {f}"
    # the host-row path on the same rows: the same bytes
    host = fmrx.Meters(IF_FS, N)
    assert host.process(iq, rows).tobytes() == got.tobytes()
    host.close()
    # the same device rows without their last samples: 74 segments and a tail, the row's own samples behind its end
    ptr, pitch, _ = bank.demod_layout()
    short = n_if - mc.D_SHORT
    meters.process_dev(None, 0, 0, ptr, pitch, short, stream=s)
    check_bits(meters.collect(), models(("d", short), rows[:, :short], table), short, f"{mc.D_SHORT} samples short")
    # the comparison's power on these very rows (the tail's place shows in a total only by luck: tests/_meters_exact_cases.py)
    want_short = models(("d", short), None, None)[0]
    for mutant in om.MUTANTS:
        fields = mc.differing_fields(om.mpx_ordered(rows[0, :short], *table, mutant), want_short)
        print(f"{mutant}: {', '.join(fields) or 'no field'} differ on channel 0")
        assert fields or mutant not in ROBUST_MUTANTS, mutant
    meters.close()
    bank.close()
