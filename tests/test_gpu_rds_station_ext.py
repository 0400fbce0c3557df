"""Burst error correction and extension records of the RDS bank's lane-per-channel station decoders
(fmrx_rds_bank_set_station_options / _stations_ext): after every call, every channel's station record, extension record and
groups must equal, byte for byte, what a host decoder with the same option (fmrx_rds_station_set_correction) makes of the
channel's matched-filter rows as collect returns them.

70 channels (a full wave of lanes and a partial one), blocks of 9 600 samples, 52 calls: two passes of the group schedule of
rds_groups_ext (0A x 4, 2A x 2, 1A, 1A, 4A, 10A x 2 = 0.96 s).  Channel c carries exact bit errors by c % 4: none; one wrong
bit in every third block; a 2-bit burst in every fifth block (at a bit of the block that depends on c; those of channels 2 and 54 straddle
into the next block, which leaves the three clean blocks in five that acquisition needs two of); a 5-bit burst in every fifth block during the first 0.6 s (beyond max_burst 2, so those blocks are lost and the
channel needs the clean second pass).  Chip offsets, chip rates, amplitudes and noise differ per channel as in
_rds_util.station_rows; channel SILENT is all zeros, channel LATE starts after 5.5 calls."""
import functools

import numpy as np
import pytest

import _rds_station_model as M
import rds_groups as RG
import rds_groups_ext as GE
from _rds_util import BLOCK, LATE, N, SILENT, channel_station

pytestmark = pytest.mark.gpu

CALLS = 52


def ext_station(c):
    s = channel_station(c)
    return dict(pi=s["pi"], pty=s["pty"], ps=s["ps"], rt=f"CH{c:03d} RT", af=(88.1 + 0.2 * (c % 50), 100.0 + 0.1 * (c % 30)), di=c & 15,
                ecc=0xE0 + c % 5, lang=1 + c % 40, pin=0x0800 + c, ct=(58000 + c, (c * 5) % 24, c % 60, (c % 2) << 5 | c % 25),
                ptyn=f"PTY{c:03d}  ")


def turns_one_offset_into_another(burst, at):
    """The syndromes of the five offset words differ pairwise by the syndromes of short bursts (A / B: bits 6-7 of the block,
    C / D: bit 7 alone, A / D: bits 1-2, ...; tests/test_rds_station_ext_host.py lists them), so a block of one offset with
    that burst IS a clean block of the other offset: no receiver can tell, and a stream with it in every third block is a
    station that sends wrong offset words, not one with reception errors.  True for the part of the burst in either block
    where it straddles a boundary."""
    syn = [0x3D8, 0x3D4, 0x25C, 0x3CC, 0x258]
    diffs = {a ^ b for a in syn for b in syn if a != b}
    here = sum(int(v) << (25 - at - k) for k, v in enumerate(burst) if at + k < 26)
    there = sum(int(v) << (25 - (at + k - 26)) for k, v in enumerate(burst) if at + k >= 26)
    return M.syndrome(here) in diffs or M.syndrome(there) in diffs


def burst_of(c):
    """-> (the burst's bits, its first bit in the block): a position that depends on the channel, the first one from (a
    multiple of c) mod 26 on that does not turn an offset word into another."""
    kind = c % 4
    length = (0, 1, 2, 5)[kind]
    inner = [c & 1, (c >> 1) & 1, (c >> 2) & 1] if kind == 3 else None
    burst = [1] * length if inner is None else [1] + inner + [1]
    at = ((0, 5, 7, 1)[kind] * c + (0, 0, 11, 0)[kind]) % (22 if kind == 3 else 26)   # (channels 2 and 54: bit 25, into the next block)
    while turns_one_offset_into_another(burst, at):
        at = (at + 1) % 26
    return burst, at


def error_pattern(c, n_bits):
    kind = c % 4
    if kind == 0:
        return np.zeros(0, np.uint8)
    burst, at = burst_of(c)
    if kind == 3:
        return GE.burst_pattern(700, 5, 5, first_block=2, at=at, inner=burst[1:-1])
    return GE.burst_pattern(n_bits, 3 if kind == 1 else 5, len(burst), first_block=1, at=at)


@functools.lru_cache(maxsize=None)
def ext_rows():
    n = CALLS * BLOCK
    rows = []
    for c in range(N):
        s = ext_station(c)
        bits = RG.stream_bits(GE.station_schedule(s["pi"], s["pty"], s["ps"], s["rt"], 3, **{k: s[k] for k in ("af", "di", "ecc", "lang", "pin", "ct", "ptyn")}))
        assert len(bits) >= n / 240e3 * 2375.0 / 2 + 8, "long enough that modulate does not tile it"
        rows.append(RG.modulate(GE.with_errors(bits, error_pattern(c, len(bits))), n, amplitude=0.04 + 0.01 * (c % 5), noise=0.002 * (c % 4),
                                chip_offset=float((53 * c) % 211), chip_rate=2375.0 * (1 + (c % 7 - 3) * 40e-6), seed=300 + c))
    rows = np.stack(rows)
    rows[SILENT] = 0.0
    rows[LATE, :11 * BLOCK // 2] = 0.0
    rows.setflags(write=False)
    return rows


def run_bank_and_host(fmrx, mode, max_burst, rows, n_calls, reset_at=None):
    n = rows.shape[0]
    bank = fmrx.RdsBank(mode, n, BLOCK)
    bank.set_stations(True, max_burst=max_burst, ext=True)
    hosts = [fmrx.RdsStationDecoder(mode, max_burst=max_burst) for _ in range(n)]
    recs = ext = None
    for b in range(n_calls):
        if reset_at is not None and b == reset_at[0]:
            bank.reset(reset_at[1])
            hosts[reset_at[1]].reset()
        got = bank.process(rows[:, b * BLOCK:(b + 1) * BLOCK])
        recs, groups = bank.stations(raw=True)
        ext = bank.stations_ext(raw=True)
        for c in range(n):
            _, g = hosts[c].feed_rrc(got["rrc_i"][c])
            assert recs[c].tobytes() == hosts[c].record.tobytes(), f"mode {mode} call {b} channel {c}: station record"
            assert ext[c].tobytes() == hosts[c].ext.tobytes(), f"mode {mode} call {b} channel {c}: extension record"
            assert groups[c].tobytes() == g.tobytes(), f"mode {mode} call {b} channel {c}: groups"
    return bank, recs, ext


@pytest.mark.parametrize("max_burst", [2, 5])
@pytest.mark.parametrize("mode", [0, 2])
def test_bank_equals_the_host_decoder(fmrx, mode, max_burst):
    bank, recs, ext = run_bank_and_host(fmrx, mode, max_burst, ext_rows(), CALLS)
    for c in range(N):
        st, x = fmrx.rds_station_dict(recs[c]), fmrx.rds_station_ext_dict(ext[c])
        assert x["max_burst"] == max_burst
        if c == SILENT:
            assert st["blocks"] == 0 and x["group_types"] == [] and x["ct"] is None and x["corrected_blocks"] == 0, (c, st, x)
            continue
        s = ext_station(c)
        where = (mode, max_burst, c, st, x)
        assert (st["pi"], st["pty"], st["ps"], st["rt"]) == (s["pi"], s["pty"], s["ps"], s["rt"].ljust(64)), where
        assert x["ct"] is not None and (x["ct"]["mjd"], x["ct"]["hour"], x["ct"]["minute"]) == s["ct"][:3], where
        assert x["ct"]["offset_minutes"] == (-30 if c % 2 else 30) * (c % 25), where
        assert (x["ecc"], x["lang"], x["pin"]) == (s["ecc"], s["lang"], s["pin"]), where
        assert (x["ptyn"], x["ptyn_mask"]) == (s["ptyn"], 3), where
        assert x["af"] == sorted(round(f, 1) for f in s["af"]) and x["af_announced"] == 2, where
        assert (x["di"], x["di_mask"]) == (s["di"], 0xF), where
        assert x["group_types"] == ["0A", "1A", "2A", "4A", "10A"], where
        if c % 4 == 2:
            straddles = burst_of(c)[1] == 25                   # one wrong bit in either block then
            assert x["corrected_blocks"] > 0 and x["burst_hist"][0 if straddles else 1] > 0, where
        if c % 4 == 1:
            assert x["burst_hist"][0] > 0, where
        if c % 4 == 3 and max_burst == 5:
            assert x["burst_hist"][4] > 0, where
    bank.close()


def test_reset_of_one_channel_clears_its_extension_record(fmrx):
    nb = 30
    bank, _, _ = run_bank_and_host(fmrx, 0, 2, ext_rows(), nb, reset_at=(8, 6))   # equality with a host decoder reset at the same call
    before = bank.stations_ext(raw=True)
    assert before[14]["corrected_blocks"] > 0 and before[14]["group_types"] != 0
    bank.reset(14)
    after = bank.stations_ext(raw=True)
    blank = fmrx.RdsStationDecoder(0, max_burst=2)
    for c in range(N):
        assert after[c].tobytes() == (blank.ext if c == 14 else before[c:c + 1]).tobytes(), c
    bank.close()


def test_options_off_changes_nothing(fmrx):
    """set_station_options(0, 0) against a bank on which it was never called: station and group bytes."""
    nb, rows = 24, ext_rows()
    for mode in (0, 2):
        plain, opt = fmrx.RdsBank(mode, N, BLOCK), fmrx.RdsBank(mode, N, BLOCK)
        plain.set_stations(True)
        opt.set_stations(True)
        assert fmrx.lib.fmrx_rds_bank_set_station_options(opt._h, 0, 0) == fmrx.OK
        n_groups = 0
        for b in range(nb):
            blk = rows[:, b * BLOCK:(b + 1) * BLOCK]
            plain.process(blk)
            opt.process(blk)
            ra, ga = plain.stations(raw=True)
            rb, gb = opt.stations(raw=True)
            assert ra.tobytes() == rb.tobytes(), (mode, b)
            for c in range(N):
                assert ga[c].tobytes() == gb[c].tobytes(), (mode, b, c)
                assert not ga[c]["reserved"].any()
                n_groups += len(ga[c])
        assert n_groups > N
        with pytest.raises(fmrx.FmrxError):
            opt.stations_ext()                                 # ext is off
        plain.close()
        opt.close()


def test_option_refusals(fmrx):
    import torch
    L = fmrx.lib
    bank = fmrx.RdsBank(0, N, BLOCK)
    x = np.zeros(N, fmrx.RDS_STATION_EXT_DTYPE)
    assert L.fmrx_rds_bank_set_station_options(bank._h, 2, 1) == fmrx.EINVAL        # stations are off
    bank.set_stations(True)
    for mb in (-1, 6):
        assert L.fmrx_rds_bank_set_station_options(bank._h, mb, 1) == fmrx.EINVAL
    assert L.fmrx_rds_bank_stations_ext(bank._h, x.ctypes.data) == fmrx.EINVAL      # ext is off
    assert L.fmrx_rds_bank_set_station_options(bank._h, 2, 0) == fmrx.OK
    assert L.fmrx_rds_bank_stations_ext(bank._h, x.ctypes.data) == fmrx.EINVAL      # still off
    assert L.fmrx_rds_bank_set_station_options(bank._h, 2, 1) == fmrx.OK
    assert L.fmrx_rds_bank_stations_ext(bank._h, None) == fmrx.EINVAL
    blank = fmrx.RdsStationDecoder(0, max_burst=2)
    assert bank.stations_ext(raw=True).tobytes() == blank.ext.tobytes() * N          # a fresh bank: fresh records
    d = torch.zeros(N * BLOCK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bank.process_dev(d.data_ptr(), BLOCK)
    with pytest.raises(fmrx.FmrxError):
        bank.process_dev(d.data_ptr(), BLOCK)                  # not collected yet
    bank.stations_ext()                                        # takes the call off the rule, as stations() does
    bank.process_dev(d.data_ptr(), BLOCK)
    bank.collect()
    assert L.fmrx_rds_bank_set_station_options(bank._h, 0, 0) == fmrx.EINVAL        # no longer fresh
    bank.reset(3)
    assert L.fmrx_rds_bank_set_station_options(bank._h, 0, 0) == fmrx.EINVAL        # one channel's reset is not a fresh bank
    bank.reset()
    bank.set_stations(True, max_burst=5, ext=True)              # right after reset(-1): allowed
    assert all(r["max_burst"] == 5 for r in bank.stations_ext())
    bank.close()
