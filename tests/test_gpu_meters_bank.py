"""The meters behind a bank, on one stream: a wide capture of three RDS stations over noise -> tuner (8 channels) -> fast
stereo bank of mode 0 -> Meters.for_bank.  Channels 0-2 sit on the stations, channel 3 on station 1 mistuned by 20 kHz,
channels 4-7 on empty offsets.  (a) every record of the last call equals the model evaluated on the slot bytes and the
discriminator rows read back; (b)-(d) the levels tell stations from empty channels, read the mistuning and the pilot's
deviation (properties of the definition: tests/test_meters_model_host.py states them on the CPU models, DESIGN.md section
4.11 records the margins); (e) the fused mono bank keeps no rows: the RF group alone."""
import numpy as np
import pytest

import _meters_capture as MC
import _meters_model as mm
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu

REL, RF_FIELDS = mm.REL, mm.RF_FIELDS

DB_LEVELS = ("level_dbfs", "cnr_db", "pilot_db", "rds_db")
PILOT_MARGIN = 0.056   # (d): the CPU models read 3.5 - 3.6 % below the generator's 0.1 rad on the last call; that + 2 %


class _DeviceBytes:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def slot_bytes(torch, first, pitch, n_bytes):
    """the block regions of the bank's N input slots, read back: uint8 [N][n_bytes]"""
    whole = torch.as_tensor(_DeviceBytes(first, (N - 1) * pitch + n_bytes), device="cuda")
    return np.stack([whole[c * pitch:c * pitch + n_bytes].cpu().numpy() for c in range(N)])


def run_chain(fmrx, oracle, stereo):
    with bank_chain(fmrx, oracle, fused_mono=not stereo) as ch:
        bank, bb = ch.bank, MC.BYTES_PER_CALL
        meters = fmrx.Meters.for_bank(bank)
        for i in ch.calls():
            meters.process_bank(stream=ch.s)
            recs = meters.collect()
        ch.stream.synchronize()
        out = dict(recs=recs, levels=[meters.derive(r) for r in recs], slots=slot_bytes(ch.torch, ch.first, ch.pitch, bb),
                   power=ch.tuner.levels()[1], rows=[bank.read_tap(k, "demod") for k in range(N)] if stereo else None,
                   if_Fs=float(bank.params.if_Fs))
        meters.close()
    return out


@pytest.fixture(scope="module")
def stereo_chain(fmrx, oracle):
    return run_chain(fmrx, oracle, True)


def test_a_records_equal_the_model_on_the_slots_and_rows(stereo_chain):
    ch = stereo_chain
    assert ch["if_Fs"] == 240000.0
    got = ch["recs"]
    want = np.array([mm.record(ch["slots"][k], ch["rows"][k], ch["if_Fs"]) for k in range(N)])
    for f in RF_FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["m2"], ch["power"])        # the tuner's own power reading of the bytes it wrote
    for f in ("n_if", "segments", "max_abs"):
        assert np.array_equal(got[f], want[f]), f
    assert got["n_if"][0] == 9600 and got["segments"][0] == 9
    for k in range(N):
        assert np.isfinite(ch["rows"][k]).all()
        e = mm.mpx_group(ch["rows"][k], ch["if_Fs"])
        assert abs(got["sum_x"][k] - want["sum_x"][k]) <= REL * e["sum_abs"]
        assert abs(got["sum_x2"][k] - want["sum_x2"][k]) <= REL * want["sum_x2"][k]
        assert np.all(np.abs(got["probe"][k] - want["probe"][k]) <= REL * e["bound"]), k
        lv, ref = ch["levels"][k], mm.derive(want[k], ch["if_Fs"])
        assert all(abs(lv[n] - ref[n]) <= 1e-6 * max(1.0, abs(ref[n])) for n in mm.LEVEL_NAMES), k


def test_b_stations_stand_out_from_empty_channels(stereo_chain):
    L = stereo_chain["levels"]
    for n in DB_LEVELS:
        empty = max(L[k][n] for k in range(4, 8))
        print(f"{n}: stations {[round(L[k][n], 2) for k in range(3)]}, empty channels at most {empty:.2f}")
        assert all(L[k][n] > empty for k in range(3)), n


def test_c_the_mistuned_channel_reads_its_offset(stereo_chain):
    """sin and tan of 2 pi 20 / 240 give 19.1 and 22.0 kHz, the two forms a differentiating discriminator can take"""
    L = stereo_chain["levels"]
    d = L[3]["freq_offset_hz"] - L[1]["freq_offset_hz"]
    print(f"freq_offset_hz: channel 3 {L[3]['freq_offset_hz']:.1f}, channel 1 {L[1]['freq_offset_hz']:.1f}")
    assert 15000.0 <= d <= 25000.0


def test_d_pilot_deviation_of_the_stations(stereo_chain):
    L = stereo_chain["levels"]
    want = 0.1 * stereo_chain["if_Fs"] / (2 * np.pi)
    rel = [L[k]["pilot_dev_hz"] / want - 1.0 for k in range(3)]
    print("pilot_dev_hz relative to the generator's 0.1 rad: " + ", ".join(f"{r:+.4f}" for r in rel))
    assert all(abs(r) <= PILOT_MARGIN for r in rel)


def test_e_the_fused_mono_bank_gives_the_rf_group_alone(fmrx, oracle, stereo_chain):
    mono = run_chain(fmrx, oracle, False)
    assert np.array_equal(mono["slots"], stereo_chain["slots"])
    zero = np.zeros(N, mm.METER_DTYPE)
    for f in RF_FIELDS:
        assert np.array_equal(mono["recs"][f], stereo_chain["recs"][f]), f
    for f in ("n_if", "segments", "sum_x", "sum_x2", "max_abs", "probe"):
        assert np.array_equal(mono["recs"][f], zero[f]), f
