"""RDS station decoding on the device: the single-stream handle's matched-filter rows into the host decoder, and the RDS bank's
lane-per-channel decoder (fmrx_rds_bank_set_stations / _stations), whose station and group records must equal, byte for byte,
what the host decoder (fmrx_rds_station_feed_rrc) makes of the same channel's rows as collect returns them."""
import numpy as np
import pytest

import rds_groups as RG
from _rds_util import BLOCK, LATE, N, SILENT, channel_station, station_rows

pytestmark = pytest.mark.gpu


def run_bank_and_host(fmrx, mode, rows, n_blocks, reset_at=None):
    n = rows.shape[0]
    bank = fmrx.RdsBank(mode, n, BLOCK)
    bank.set_stations(True)
    hosts = [fmrx.RdsStationDecoder(mode) for _ in range(n)]
    last = None
    for b in range(n_blocks):
        if reset_at is not None and b == reset_at[0]:
            bank.reset(reset_at[1])
            hosts[reset_at[1]].reset()
        got = bank.process(rows[:, b * BLOCK:(b + 1) * BLOCK])
        recs, groups = bank.stations(raw=True)
        for c in range(n):
            _, g = hosts[c].feed_rrc(got["rrc_i"][c])
            assert recs[c].tobytes() == hosts[c].record.tobytes(), f"mode {mode} call {b} channel {c}: station record"
            assert groups[c].tobytes() == g.tobytes(), f"mode {mode} call {b} channel {c}: groups"
        last = recs
    return bank, last


def test_single_stream_handle_and_host_decoder(fmrx):
    s = dict(pi=0xD3A2, pty=5, ps="CLASSIC ", rt="NOW PLAYING: SOMETHING")
    x = RG.station_demod(50 * BLOCK, chip_rate=2375.0 * (1 - 120e-6), chip_offset=400.0, amplitude=0.05, noise=0.003, **s)
    rds, dec = fmrx.Rds(0, max_block=BLOCK), fmrx.RdsStationDecoder(0)
    for b in range(50):
        st, _ = dec.feed_rrc(rds.process(x[b * BLOCK:(b + 1) * BLOCK])["rrc_i"])
    assert (st["pi"], st["pty"], st["ps"], st["rt"]) == (s["pi"], s["pty"], s["ps"], s["rt"].ljust(64)), st
    assert st["synced"] and st["good_blocks"] >= 0.99 * st["blocks"]


@pytest.mark.parametrize("mode", [0, 2])
def test_bank_stations_equal_the_host_decoder(fmrx, mode):
    nb = 36
    rows = station_rows(nb)
    bank, recs = run_bank_and_host(fmrx, mode, rows, nb)
    st = [fmrx.rds_station_dict(r) for r in recs]
    for c in range(N):
        if c == SILENT:
            assert not st[c]["synced"] and st[c]["blocks"] == 0 and st[c]["groups"] == 0, st[c]
            continue
        s = channel_station(c)
        assert (st[c]["pi"], st[c]["pty"], st[c]["ps"]) == (s["pi"], s["pty"], s["ps"]), (mode, c, st[c])
        assert st[c]["rt"] == s["rt"].ljust(64), (mode, c, st[c])
    bank.close()


def test_bank_reset_of_one_channel(fmrx):
    nb = 30
    rows = station_rows(nb)
    bank, recs = run_bank_and_host(fmrx, 0, rows, nb, reset_at=(6, 7))    # equality with a host decoder reset at the same call
    st = fmrx.rds_station_dict(recs[7])
    assert st["ps"] == channel_station(7)["ps"]
    # a reset right before reading: only that channel's record is cleared
    before, _ = bank.stations(raw=True)
    bank.reset(12)
    after, groups = bank.stations(raw=True)
    blank = fmrx.RdsStationDecoder(0)
    blank.feed_bits([])
    for c in range(N):
        if c == 12:
            assert after[c].tobytes() == blank.record.tobytes() and len(groups[c]) == 0
        else:
            assert after[c].tobytes() == before[c].tobytes(), c
    bank.close()


def test_stations_off_changes_nothing(fmrx):
    nb = 4
    rows = station_rows(nb)
    for mode in (0, 2):
        off, on = fmrx.RdsBank(mode, N, BLOCK), fmrx.RdsBank(mode, N, BLOCK)
        on.set_stations(True)
        for b in range(nb):
            blk = rows[:, b * BLOCK:(b + 1) * BLOCK]
            a, c = off.process(blk), on.process(blk)
            for ch in range(N):
                for k in ("rrc_i", "rrc_q", "diff_bits"):
                    assert np.array_equal(np.asarray(a[k][ch]).view(np.uint8), np.asarray(c[k][ch]).view(np.uint8)), (mode, b, ch, k)
                assert a["offset_type"][ch] == c["offset_type"][ch]
        with pytest.raises(fmrx.FmrxError):
            off.stations()                                  # stations are off
        off.close()
        on.close()


def test_receiver_bank_to_stations_on_the_device(fmrx):
    """u8 I/Q -> exact stereo receiver bank -> fmrx_channels_demod_layout -> RDS bank with stations, all on the device."""
    import torch
    n, nb = 3, 36
    stations = [dict(pi=0xA100 + c, pty=3 + c, ps=["ALPHA FM", "BRAVO   ", "CHARLIE "][c], rt=f"TEXT OF STATION {c}") for c in range(n)]
    iqs = [RG.station_iq_u8(nb * BLOCK * 10, chip_offset=800.0 + 131 * c, seed=40 + c, **stations[c]) for c in range(n)]
    ch = fmrx.Channels(0, n, audio_channels=2, exact=True, block_bytes=192000)
    stream = torch.cuda.Stream()
    d_iq = torch.from_numpy(np.stack(iqs)).cuda()
    audio = torch.zeros(n * ch.audio_channels * ch.n_audio, dtype=torch.float32, device="cuda")
    pcm = torch.zeros(n * ch.audio_channels * ch.n_audio, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ptr, pitch, n_if = ch.demod_layout()
    assert n_if == BLOCK
    bank = fmrx.RdsBank(0, n, n_if)
    bank.set_stations(True)
    for b in range(nb):
        blk = d_iq[:, b * 192000:(b + 1) * 192000].contiguous()
        torch.cuda.synchronize()
        ch.load_dev(blk.data_ptr(), stream=stream.cuda_stream)
        ch.process_dev(audio.data_ptr(), pcm.data_ptr(), stream=stream.cuda_stream)
        bank.process_dev(ptr, pitch, stream=stream.cuda_stream)
        st, _ = bank.stations()
    for c in range(n):
        assert (st[c]["pi"], st[c]["pty"], st[c]["ps"]) == (stations[c]["pi"], stations[c]["pty"], stations[c]["ps"]), (c, st[c])
        assert st[c]["rt"] == stations[c]["rt"].ljust(64), (c, st[c])
    bank.close()
    ch.close()


def test_station_refusals(fmrx):
    import torch
    bank = fmrx.RdsBank(0, N, BLOCK)
    d = torch.zeros(N * BLOCK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bank.process_dev(d.data_ptr(), BLOCK)
    bank.collect()
    with pytest.raises(fmrx.FmrxError):
        bank.set_stations(True)                             # after the first call
    bank.reset(3)
    with pytest.raises(fmrx.FmrxError):
        bank.set_stations(True)                             # a reset of one channel is not a fresh bank
    bank.reset()
    bank.set_stations(True)                                 # right after reset(-1): allowed
    rec = np.zeros(N, fmrx.RDS_STATION_DTYPE)
    g = np.zeros((N, bank.max_groups), fmrx.RDS_GROUP_DTYPE)
    ng = np.zeros(N, np.uint64)
    L = fmrx.lib
    assert L.fmrx_rds_bank_stations(bank._h, None, g.ctypes.data, ng.ctypes.data) == fmrx.EINVAL   # no station records
    assert L.fmrx_rds_bank_stations(bank._h, rec.ctypes.data, g.ctypes.data, None) == fmrx.EINVAL  # groups without counts
    bank.process_dev(d.data_ptr(), BLOCK)
    with pytest.raises(fmrx.FmrxError):
        bank.process_dev(d.data_ptr(), BLOCK)               # not collected yet
    assert L.fmrx_rds_bank_stations(bank._h, rec.ctypes.data, None, None) == fmrx.OK   # stations() takes it off the rule
    bank.process_dev(d.data_ptr(), BLOCK)
    bank.collect()                                          # and so does collect()
    st, groups = bank.stations()
    assert all(not s["synced"] and s["blocks"] == 0 for s in st) and all(len(x) == 0 for x in groups)
    with pytest.raises(fmrx.FmrxError):
        bank.set_stations(False)                            # no longer fresh
    bank.close()
