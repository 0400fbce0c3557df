"""RDS station decoder on the host (fmrx_rds_station_*, RdsStationDecoder): no GPU needed.

The library's decoder (rds_station.hpp) is compared byte for byte -- station records and group records -- with its pure-Python
restatement (_rds_station_model.py) on bit streams (clean, with bit errors, with a slipped bit, behind garbage, version-B groups,
an A/B text toggle) and on matched-filter rows of the CPU oracle's RDS chain; then the decoder is checked for what it is for:
through the oracle chain, a station's PI, PTY, PS and RadioText come out, at chip rates off by up to +-150 ppm."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _rds_station_model as M  # noqa: E402
import rds_groups as RG  # noqa: E402

PI, PTY, PS, RT = 0xC201, 10, "TESTFM  ", "HELLO RDS WORLD!"
BLOCK = 9600
MODES = {0: (247, 960, 26), 2: (817, 1920, 43)}


def same_as_model(fmrx, dec, model, chunks, kind):
    """Feeds the same chunks to the library's decoder and the model; every record and every group byte for byte."""
    out = []
    for ch in chunks:
        if kind == "bits":
            st, g = dec.feed_bits(ch)
            rec, mg = model.feed_bits(ch)
        else:
            st, g = dec.feed_rrc(ch)
            rec, mg = model.feed_rrc(ch)
        assert dec.record.tobytes() == rec, (st, M.StationModel.__name__)
        assert g.tobytes() == b"".join(mg), (len(g), len(mg))
        out.append((st, g))
    return out


def chunks_of(x, n):
    return [x[i:i + n] for i in range(0, len(x), n)]


def station_bits(n_groups, **kw):
    return RG.stream_bits(RG.station_groups(PI, PTY, PS, RT, n_groups, **kw))


def check_station(st, ps=PS, rt=RT, pi=PI, pty=PTY):
    assert (st["pi"], st["pty"], st["ps"], st["rt"]) == (pi, pty, ps, rt.ljust(64)), st
    assert st["ps_mask"] == 0xF and st["seen"] == 3


def test_record_layout_matches_the_header(fmrx):
    """fmrx_rds_station / fmrx_rds_group as include/fmrx.h declares them (laid out by ctypes, i.e. by the C rules) against the
    numpy dtypes the Python layer reads them with, and the sizes the header's static asserts fix."""
    hdr = open(os.path.join(ROOT, "include", "fmrx.h")).read()
    ctypes_of = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "char": C.c_char}
    for name, dt in (("fmrx_rds_station", fmrx.RDS_STATION_DTYPE), ("fmrx_rds_group", fmrx.RDS_GROUP_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = []
        for line in body.splitlines():
            m = re.match(r"\s*(\w+)\s+([^;]+);", line)
            if not m:
                continue
            for decl in m.group(2).split(","):
                dm = re.match(r"\s*(\w+)(?:\[(\d+)\])?", decl)
                t = ctypes_of[m.group(1)]
                fields.append((dm.group(1), t * int(dm.group(2)) if dm.group(2) else t))
        S = type(name, (C.Structure,), {"_fields_": fields})
        size = int(re.search(r"sizeof\(%s\) == (\d+)" % name, hdr).group(1))
        assert C.sizeof(S) == dt.itemsize == size, (name, C.sizeof(S), dt.itemsize, size)
        assert [f[0] for f in fields] == list(dt.names), name
        for f, _ in fields:
            assert getattr(S, f).offset == dt.fields[f][1], (name, f)


def test_api(fmrx):
    lib = C.CDLL(fmrx.LIB_PATH)
    for sym in ("fmrx_rds_station_create", "fmrx_rds_station_destroy", "fmrx_rds_station_reset", "fmrx_rds_station_max_groups",
                "fmrx_rds_station_feed_rrc", "fmrx_rds_station_feed_bits", "fmrx_rds_bank_set_stations", "fmrx_rds_bank_stations",
                "fmrx_rds_bank_max_groups"):
        assert hasattr(lib, sym), sym
    for name in ("set_stations", "stations"):
        assert callable(getattr(fmrx.RdsBank, name)), name
    L, h = fmrx.lib, C.c_void_p()
    for sps in (1, 65):
        assert L.fmrx_rds_station_create(C.byref(h), sps) == fmrx.EINVAL
    assert L.fmrx_rds_station_create(None, 26) == fmrx.EINVAL
    n = C.c_size_t(0)
    rec = np.zeros(1, fmrx.RDS_STATION_DTYPE)
    g = np.zeros(4, fmrx.RDS_GROUP_DTYPE)
    assert L.fmrx_rds_station_feed_bits(None, None, 0, None, 0, None, rec.ctypes.data) == fmrx.EINVAL
    assert L.fmrx_rds_station_create(C.byref(h), 26) == fmrx.OK
    assert L.fmrx_rds_station_feed_bits(h, None, 0, None, 0, None, None) == fmrx.EINVAL           # no record
    assert L.fmrx_rds_station_feed_bits(h, None, 0, g.ctypes.data, 4, None, rec.ctypes.data) == fmrx.EINVAL   # g without n_g
    assert L.fmrx_rds_station_feed_rrc(h, None, 5, None, 0, None, rec.ctypes.data) == fmrx.EINVAL   # no row
    assert L.fmrx_rds_station_feed_bits(h, None, 0, g.ctypes.data, 4, C.byref(n), rec.ctypes.data) == fmrx.OK and n.value == 0
    assert L.fmrx_rds_station_max_groups(h, 2470) == M.max_groups_for_samples(2470, 26)
    assert L.fmrx_rds_station_destroy(h) == fmrx.OK
    # a fresh record: nothing decoded, text all spaces
    d = fmrx.RdsStationDecoder(0)
    st, g = d.feed_bits([])
    assert len(g) == 0 and st["ps"] == " " * 8 and st["rt"] == " " * 64 and st["rt_ab"] == 2 and not st["synced"]
    assert d.record.tobytes() == M.StationModel(26).record()
    for L_ in (None,):
        assert fmrx.lib.fmrx_rds_bank_set_stations(L_, 1) == fmrx.EINVAL
        assert fmrx.lib.fmrx_rds_bank_stations(L_, None, None, None) == fmrx.EINVAL
        assert fmrx.lib.fmrx_rds_bank_max_groups(L_) == 0


def test_clean_bits(fmrx):
    bits = station_bits(16)
    dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
    out = same_as_model(fmrx, dec, model, chunks_of(bits[7:], 190), "bits")   # starts mid-block
    st = out[-1][0]
    check_station(st)
    assert st["synced"] and st["good_blocks"] == st["blocks"]
    groups = np.concatenate([g for _, g in out])
    assert len(groups) == st["groups"] >= 14
    assert groups["ok_mask"][0] == 0xE                                      # acquired on A -> B: A's block was cut by the start
    assert np.all(groups["ok_mask"][1:] & 0xF == 0xF)
    assert np.all(np.diff(groups["bit_index"][1:].astype(np.int64)) == 104)
    assert groups["bit_index"][1] == 104 - 7                                # the groups sit where they were sent
    assert groups["bit_index"][0] == (-7) % (1 << 32)                       # (the first one began before the stream)
    assert np.all(groups["block"][1:, 0] == PI)
    dec.reset()
    st, g = dec.feed_bits(bits)
    check_station(st)


def test_random_bit_errors(fmrx):
    rng = np.random.default_rng(7)
    bits = station_bits(48)
    for ber in (0.002, 0.01, 0.03):
        noisy = bits ^ (rng.random(len(bits)) < ber).astype(np.uint8)
        dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
        out = same_as_model(fmrx, dec, model, chunks_of(noisy, 97), "bits")
        st = out[-1][0]
        assert st["good_blocks"] < st["blocks"] or ber < 0.005
        if ber <= 0.01:
            check_station(st)


@pytest.mark.parametrize("slip", ["insert", "delete"])
def test_slipped_bit_reacquires_within_three_groups(fmrx, slip):
    bits = station_bits(40)
    P = 20 * 104 + 37
    slipped = np.concatenate([bits[:P], [1], bits[P:]]) if slip == "insert" else np.concatenate([bits[:P], bits[P + 1:]])
    dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
    out = same_as_model(fmrx, dec, model, chunks_of(slipped, 113), "bits")
    groups = np.concatenate([g for _, g in out])
    gi = groups["bit_index"].astype(np.int64)
    full = (groups["ok_mask"] & 0xF) == 0xF
    assert np.all(full[gi + 104 <= P]), "before the slip every group is whole"
    assert np.any(~full[(gi < P + 3 * 104) & (gi + 104 > P)]), "the slip is seen"
    assert np.all(full[gi >= P + 3 * 104]), "re-acquired within three groups"
    after = gi[gi >= P + 3 * 104]
    assert len(after) >= 15 and np.all(np.diff(after) == 104)
    assert (after[0] - (1 if slip == "insert" else -1)) % 104 == 0        # on the new grid
    check_station(out[-1][0])


def test_garbage_before_the_first_group(fmrx):
    rng = np.random.default_rng(11)
    garbage = (rng.random(1000) < 0.5).astype(np.uint8)
    bits = np.concatenate([garbage, station_bits(20)])
    dec, model = fmrx.RdsStationDecoder(2), M.StationModel(43)
    out = same_as_model(fmrx, dec, model, chunks_of(bits, 150), "bits")
    groups = np.concatenate([g for _, g in out])
    assert groups["bit_index"].min() >= 1000 - 104
    assert np.all((groups["bit_index"] - 1000) % 104 == 0)
    check_station(out[-1][0])


def test_version_b_groups_and_c_prime(fmrx):
    """0B and 2B groups (C' carries the PI); with every block A damaged, the PI comes from C' alone."""
    rt = "VERSION B TEXT"
    bits = RG.stream_bits(RG.station_groups(PI, PTY, PS, rt, 24, version="B", rt_version="B"))
    for damage_a in (False, True):
        b = bits.copy()
        if damage_a:
            b[np.arange(0, len(b), 104) + 3] ^= 1
        dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
        out = same_as_model(fmrx, dec, model, chunks_of(b, 200), "bits")
        st = out[-1][0]
        groups = np.concatenate([g for _, g in out])
        assert np.all(groups["ok_mask"][-10:] & 0x10), "slot 2 carried C'"
        assert (st["pi"], st["pty"], st["ps"], st["rt"]) == (PI, PTY, PS, rt.ljust(32).ljust(64)), st
        assert st["rt_mask"] == (1 << 7) - 1
        if damage_a:
            assert np.all(groups["ok_mask"] & 1 == 0)


def test_text_ab_toggle(fmrx):
    first, second = "FIRST RADIOTEXT MESSAGE ON AIR..", "SECOND ONE"
    bits = np.concatenate([RG.stream_bits(RG.station_groups(PI, PTY, PS, first, 24, ab=0)),
                           RG.stream_bits(RG.station_groups(PI, PTY, PS, second, 12, ab=1))])
    dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
    out = same_as_model(fmrx, dec, model, chunks_of(bits, 24 * 104), "bits")
    assert out[0][0]["rt"] == first.ljust(64) and out[0][0]["rt_ab"] == 0 and out[0][0]["rt_mask"] == 0xFF
    assert out[1][0]["rt"] == second.ljust(64) and out[1][0]["rt_ab"] == 1 and out[1][0]["rt_mask"] == 0x7


def oracle_rrc(mode, seconds, **kw):
    """The station's fm_demod through the CPU oracle's RDS chain in 9 600-sample calls -> the in-phase matched-filter rows."""
    import rds_oracle as R
    U, D, sps = MODES[mode]
    x = RG.station_demod(int(240000 * seconds), **kw)
    chain = R.RdsChain(upsamp=U, decim=D, sps=sps)
    return [chain.process(x[i:i + BLOCK])["rrc_i"] for i in range(0, len(x) - BLOCK + 1, BLOCK)]


def test_feed_rrc_equals_the_model(fmrx):
    rows = oracle_rrc(0, 1.2, chip_rate=2375 * (1 + 150e-6), chip_offset=311.0, noise=0.01, amplitude=0.05)
    rng = np.random.default_rng(3)
    rows = rows + [rng.standard_normal(2470) * 0.02 for _ in range(4)]      # and noise alone: the tracker wanders
    dec, model = fmrx.RdsStationDecoder(0), M.StationModel(26)
    out = same_as_model(fmrx, dec, model, rows, "rrc")
    assert any(st["synced"] for st, _ in out)


@pytest.mark.parametrize("ppm", [0, 150, -150])
@pytest.mark.parametrize("mode", [0, 2])
def test_station_through_the_oracle_chain(fmrx, mode, ppm):
    """5 s of a station through the oracle's RDS chain, chips off by ppm, fed in the 9 600-sample calls of the RDS path.
    Measured when this test was written (all six cases alike): PI, PTY, PS and RT right from the 17th call (0.68 s); 161 of
    161 blocks good over the last 3.5 s.  Required: right after 1.5 s, >= 99 % of the blocks good after it."""
    rows = oracle_rrc(mode, 5.0, chip_rate=2375 * (1 + ppm * 1e-6), chip_offset=600.0)
    dec = fmrx.RdsStationDecoder(mode)
    hist = [dec.feed_rrc(r)[0] for r in rows]
    k = int(round(1.5 / (BLOCK / 240e3)))
    for st in hist[k - 1:]:
        check_station(st)
    blocks = hist[-1]["blocks"] - hist[k - 1]["blocks"]
    good = hist[-1]["good_blocks"] - hist[k - 1]["good_blocks"]
    assert blocks >= 150 and good >= 0.99 * blocks, (good, blocks)
