"""Burst error correction and the extension record of the RDS station decoder on the host (fmrx_rds_station_set_correction,
fmrx_rds_station_ext_get, fmrx_rds_block_correct): no GPU needed.

The correction table is checked exhaustively against the model's own enumeration of bursts; the library's decoder is compared
byte for byte -- station record, extension record, groups -- with its Python restatement (_rds_station_ext_model.py) on bit
streams with exact error patterns and on noisy matched-filter rows of the CPU oracle's RDS chain; with max_burst = 0 it must be
the decoder it was before the option existed; then what the option is for (a 2-bit burst in every third block costs nothing at
max_burst 2) and the decoded values (clock time, alternative frequencies, ECC, language, PIN, PTYN, DI)."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _rds_station_ext_model as X  # noqa: E402
import _rds_station_model as M  # noqa: E402
import rds_groups as RG  # noqa: E402
import rds_groups_ext as GE  # noqa: E402

PI, PTY, PS, RT = 0xC201, 10, "TESTFM  ", "HELLO RDS WORLD!"
BURSTS = (0, 1, 2, 5)
OFFSET_NAMES = ("A", "B", "C", "Cp", "D")
STATION = dict(af=(88.1, 99.9, 107.9), di=0b1001, ecc=0xE0, lang=0x009, pin=0x5A21, ct=(0x1ABCD, 23, 59, 0x22), ptyn="FOOTBALL")


def chunks_of(x, n):
    return [x[i:i + n] for i in range(0, len(x), n)]


def uneven_chunks(x, seed=5):
    """Uneven pieces, some empty, some shorter than a block, some several groups long."""
    rng = np.random.default_rng(seed)
    out, i = [], 0
    while i < len(x):
        n = int(rng.choice([0, 1, 25, 26, 27, 103, 190, 517]))
        out.append(x[i:i + n])
        i += n
    return out


@functools.lru_cache(maxsize=None)
def streams():
    """name -> bits.  The patterns sit on the block grid of the schedule's stream, which starts on a block boundary."""
    base = RG.stream_bits(GE.station_schedule(PI, PTY, PS, RT, 4, **STATION))
    n = len(base)
    s = {"clean": base}
    s["1-bit in every third block"] = GE.with_errors(base, GE.burst_pattern(n, 3, 1, first_block=1, at=11))
    s["2-bit burst in every third block"] = GE.with_errors(base, GE.burst_pattern(n, 3, 2, first_block=1, at=7))
    s["2-bit burst across block boundaries"] = GE.with_errors(base, GE.burst_pattern(n, 3, 2, first_block=9, at=25))
    s["5-bit bursts"] = GE.with_errors(base, GE.burst_pattern(n, 3, 5, first_block=9, at=3, inner=[0, 1, 0])
                                       ^ GE.burst_pattern(n, 5, 5, first_block=10, at=21))
    s["6-bit bursts"] = GE.with_errors(base, GE.burst_pattern(n, 3, 6, first_block=9, at=3, inner=[0, 0, 0, 0]))
    # version-B groups: bursts in block B (slot 1) and in C' (slot 2), alone and together; an uncorrectable B in front of a
    # damaged C' (no correction in slot 2 then)
    vb = RG.stream_bits(RG.station_groups(PI, PTY, PS, "VERSION B TEXT", 40, version="B", rt_version="B"))
    p = np.zeros(len(vb), np.uint8)
    for g in range(8, 40):
        at = 104 * g
        if g % 4 == 0:
            p[at + 26 + 12:at + 26 + 14] = 1                       # B
        elif g % 4 == 1:
            p[at + 52 + 5:at + 52 + 7] = 1                         # C'
        elif g % 4 == 2:
            p[at + 26 + 20:at + 26 + 22] = 1                       # B and C'
            p[at + 52 + 9] = 1
        else:
            p[[at + 26 + 1, at + 26 + 9, at + 26 + 17]] = 1        # B lost
            p[at + 52 + 5:at + 52 + 7] = 1
    s["version B: errors in B and C'"] = GE.with_errors(vb, p)
    # six failed blocks in a row, then a clean stream: three wrong bits far apart in each, the first such triple whose
    # syndrome is no burst's of length <= 5 (the code is linear: that holds whatever the block carries)
    triple = next(t for t in ((2, 11 + k, 20) for k in range(8))
                  if M.syndrome(sum(1 << (25 - b) for b in t)) not in X.TABLE)
    p = np.zeros(n, np.uint8)
    for blk in range(40, 46):
        p[[26 * blk + b for b in triple]] = 1
    s["six failed blocks in a row"] = GE.with_errors(base, p)
    garbage = (np.random.default_rng(11).random(1000) < 0.5).astype(np.uint8)
    s["garbage in front"] = np.concatenate([garbage, s["2-bit burst in every third block"]])
    return s


def run_pair(fmrx, bits, max_burst, chunks=None):
    """The library's decoder and the model on the same pieces: station record, extension record and groups byte for byte after
    every piece.  -> (decoder, model, all groups)."""
    dec, model = fmrx.RdsStationDecoder(0, max_burst=max_burst), X.StationExtModel(26, max_burst)
    groups = []
    for k, ch in enumerate(uneven_chunks(bits) if chunks is None else chunks):
        _, g = dec.feed_bits(ch)
        rec, mg = model.feed_bits(ch)
        assert dec.record.tobytes() == rec, (max_burst, k, "station record")
        assert g.tobytes() == b"".join(mg), (max_burst, k, "groups")
        assert dec.ext.tobytes() == model.ext_record(), (max_burst, k, fmrx.rds_station_ext_dict(dec.ext[0]))
        groups.append(g)
    return dec, model, np.concatenate(groups)


def block_word(info, off):
    w = 0
    for b in RG.block_bits(info, OFFSET_NAMES[off]):
        w = (w << 1) | b
    return w


# ---- the correction table -------------------------------------------------------------------------------------------------

def test_burst_syndromes_are_unique_up_to_length_5():
    """The model's enumeration: bursts of length <= 1, 2, 3, 4, 5 have 26, 51, 99, 191, 367 syndromes, all distinct and
    non-zero (burst_table raises otherwise); length 6 collides."""
    for max_len, count in zip(range(1, 6), (26, 51, 99, 191, 367)):
        t = X.burst_table(max_len)
        assert len(t) == count and 0 not in t and all(0 < s < 1024 for s in t)
        assert len({p for p, _ in t.values()}) == count
    with pytest.raises(ValueError):
        X.burst_table(6)


def test_block_correct_over_every_burst(fmrx):
    L = fmrx.lib
    info, blen = C.c_uint16(0), C.c_int(0)
    n = 0
    for off in range(5):
        for word in (0x0000, 0xFFFF, 0xC201, 0x1234, 0xA5A5):
            w = block_word(word, off)
            for mb in range(6):
                assert L.fmrx_rds_block_correct(w, off, mb, C.byref(info), C.byref(blen)) == 0, "clean"
                assert (info.value, blen.value) == (word, 0)
            for pat, length in X.TABLE.values():
                for mb in range(6):
                    rc = L.fmrx_rds_block_correct(w ^ pat, off, mb, C.byref(info), C.byref(blen))
                    if length <= mb:
                        assert (rc, info.value, blen.value) == (1, word, length), (off, hex(word), hex(pat), mb)
                    else:
                        assert (rc, blen.value) == (2, 0), (off, hex(word), hex(pat), mb)
                    assert (rc, info.value, blen.value) == X.block_correct(w ^ pat, off, mb)
                    n += 1
    assert n == 367 * 5 * 5 * 6
    # a 6-bit burst is never repaired to the word that was sent
    w = block_word(0xC201, 1)
    for lo in range(0, 21):
        rc = L.fmrx_rds_block_correct(w ^ (0b100001 << lo), 1, 5, C.byref(info), C.byref(blen))
        assert rc == 2 or info.value != 0xC201                 # (where it aliases a shorter burst, the result is another word)
    assert fmrx.rds_block_correct(w ^ 0b11, 1, 2) == (1, 0xC201, 2)


def test_offset_words_differ_by_short_bursts(fmrx):
    """A property of the code and its offset words that every user of max_burst should know (rds_station.hpp):
    the offsets' syndromes differ pairwise by the syndromes of bursts -- a block of one offset with that burst is a clean block
    of the other.  Hence correction only aims at the expected offset, acquisition wants clean matches, and a lock with the
    slots one off (A taken for B, B for C, C for D, D for A: bursts of 2, 4, 1, 2) corrects every block from max_burst 4 on."""
    length = {}
    for i in range(5):
        for j in range(i + 1, 5):
            pat, n = X.TABLE.get(X.SYN_OF[i] ^ X.SYN_OF[j], (0, 0))
            length[OFFSET_NAMES[i] + OFFSET_NAMES[j]] = n
            if n:
                for word in (0x0000, 0xC201, 0xFFFF):
                    assert fmrx.rds_block_correct(block_word(word, i) ^ pat, j, 0) == (0, word ^ (pat >> 10), 0)
                    assert fmrx.rds_block_correct(block_word(word, i), j, n) == (1, word ^ (pat >> 10), n)
                    assert fmrx.rds_block_correct(block_word(word, i), j, n - 1)[0] == 2
    assert length == {"AB": 2, "AC": 0, "ACp": 3, "AD": 2, "BC": 4, "BCp": 2, "BD": 4, "CCp": 5, "CD": 1, "CpD": 3}


# ---- the decoder against the model ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_burst", BURSTS)
def test_streams_equal_the_model(fmrx, max_burst):
    for name, bits in streams().items():
        dec, model, groups = run_pair(fmrx, bits, max_burst)
        x = dec.ext[0]
        assert x["max_burst"] == max_burst and x["corrected_blocks"] == sum(x["burst_hist"]), name
        assert x["corrected_blocks"] == sum(bin(int(v)).count("1") for v in groups["reserved"][:, 0]), name
        assert np.all(groups["reserved"][:, 0] & ~groups["ok_mask"] & 0xF == 0), "a corrected block is a passed block"
        assert np.all(groups["reserved"][:, 1:] == 0)
        if max_burst == 0:
            assert x["corrected_blocks"] == 0 and np.all(groups["reserved"] == 0), name
        if name == "6-bit bursts":                                    # (this one's syndrome is no shorter burst's: never corrected)
            st = fmrx.rds_station_dict(dec.record[0])
            assert x["corrected_blocks"] == 0 and st["good_blocks"] < st["blocks"], name


@pytest.mark.parametrize("name", sorted(streams()))
def test_max_burst_0_is_the_decoder_as_it_was(fmrx, name):
    """max_burst = 0 (set explicitly, extension record read) against a decoder on which no new call is made, and against the
    model of the decoder as it was: base record and groups."""
    bits = streams()[name]
    new, old, was = fmrx.RdsStationDecoder(0), fmrx.RdsStationDecoder(0), M.StationModel(26)
    assert fmrx.lib.fmrx_rds_station_set_correction(new._h, 0) == fmrx.OK
    for ch in uneven_chunks(bits, seed=9):
        _, g = new.feed_bits(ch)
        new.ext
        _, g0 = old.feed_bits(ch)
        rec, mg = was.feed_bits(ch)
        assert new.record.tobytes() == old.record.tobytes() == rec
        assert g.tobytes() == g0.tobytes() == b"".join(mg)


def test_sync_loss_is_counted_once_and_sync_comes_back(fmrx):
    bits = streams()["six failed blocks in a row"]
    for mb in BURSTS:
        dec, model, groups = run_pair(fmrx, bits, mb)
        st, x = fmrx.rds_station_dict(dec.record[0]), fmrx.rds_station_ext_dict(dec.ext[0])
        assert x["sync_losses"] == 1 and st["synced"], (mb, x)
        gi = groups["bit_index"].astype(np.int64)
        assert np.all((groups["ok_mask"] & 0xF)[gi >= 48 * 26] == 0xF), "whole groups again after re-acquisition"
        assert gi.max() == len(bits) - 104 and np.all(gi % 104 == 0)
    # correction does not hold sync on its own: the flywheel counts only clean blocks as good evidence
    dec, _, _ = run_pair(fmrx, streams()["2-bit burst in every third block"], 2)
    assert dec.ext[0]["sync_losses"] == 0


def test_c_or_c_prime_follows_block_b(fmrx):
    bits = streams()["version B: errors in B and C'"]
    dec, _, groups = run_pair(fmrx, bits, 2, chunks=chunks_of(bits, 104))
    late = groups[groups["bit_index"] >= 8 * 104]
    assert len(late) == 32
    ok, cm = late["ok_mask"], late["reserved"][:, 0]
    k = (late["bit_index"] // 104) % 4
    assert np.all(ok[k == 0] == 0x1F) and np.all(cm[k == 0] == 0x2)            # B repaired
    assert np.all(ok[k == 1] == 0x1F) and np.all(cm[k == 1] == 0x4)            # C' repaired: bit 4 says C'
    assert np.all(ok[k == 2] == 0x1F) and np.all(cm[k == 2] == 0x6)            # both
    assert np.all(ok[k == 3] == 0x09) and np.all(cm[k == 3] == 0x0)            # B lost: C' is not tried
    assert np.all(late["block"][k < 3, 2] == PI)
    st = fmrx.rds_station_dict(dec.record[0])
    assert (st["pi"], st["ps"]) == (PI, PS)
    dec0, _, groups0 = run_pair(fmrx, bits, 0, chunks=chunks_of(bits, 104))
    late0 = groups0[groups0["bit_index"] >= 8 * 104]
    assert list(late0["ok_mask"][:4]) == [0x1D, 0x0B, 0x09, 0x09]


# ---- what it is for -------------------------------------------------------------------------------------------------------

def test_two_bit_bursts_cost_nothing_at_max_burst_2(fmrx):
    """A 2-bit burst in every third block (what one wrong chip pair in three blocks does)."""
    rt = "RADIOTEXT OF THIRTY-TWO LETTERS."
    groups = RG.station_groups(PI, PTY, PS, rt, 96)
    clean = RG.stream_bits(groups)
    bits = GE.with_errors(clean, GE.burst_pattern(len(clean), 3, 2, first_block=1, at=7))
    d0, m0, _ = run_pair(fmrx, bits, 0, chunks=chunks_of(bits, 104))
    d2, m2, _ = run_pair(fmrx, bits, 2, chunks=chunks_of(bits, 104))
    s0, s2, x2 = fmrx.rds_station_dict(d0.record[0]), fmrx.rds_station_dict(d2.record[0]), fmrx.rds_station_ext_dict(d2.ext[0])
    assert s0["blocks"] == s2["blocks"] >= 4 * 94
    assert abs(3 * s0["good_blocks"] - 2 * s0["blocks"]) <= 8, s0          # two thirds, within the first and last group
    assert s2["good_blocks"] == s2["blocks"], s2
    assert abs(3 * x2["corrected_blocks"] - s2["blocks"]) <= 8, x2          # a third, within the first and last group
    assert x2["burst_hist"] == [0, x2["corrected_blocks"], 0, 0, 0]
    assert (s2["ps"], s2["rt"], s2["ps_mask"], s2["rt_mask"]) == (PS, rt.ljust(64), 0xF, 0xFF), s2

    def groups_until_complete(mb):
        m = X.StationExtModel(26, mb)
        for k, ch in enumerate(chunks_of(bits, 104)):
            m.feed_bits(ch)
            if m.ps_mask == 0xF and m.rt_mask == 0xFF:
                return k + 1
        return None
    n0, n2 = groups_until_complete(0), groups_until_complete(2)
    print(f"groups until PS and RT are whole: max_burst 0: {n0}, max_burst 2: {n2}")
    assert n2 is not None and (n0 is None or n0 >= 2 * n2)      # (None: with this pattern no 2A group ever has B, C and D whole)


# ---- decoded values -------------------------------------------------------------------------------------------------------

def test_decoded_values(fmrx):
    groups = GE.station_schedule(PI, PTY, PS, RT, 2, **STATION)
    groups.append(GE.group_0a(PI, PTY, PS, 0, (250, 17), di=STATION["di"]))        # an LF/MF frequency: the low byte is not a code
    groups.append(GE.group_4a(PI, PTY, 60000, 24, 0, 0))                            # hour 24: not a time
    groups.append(GE.group_4a(PI, PTY, 60000, 12, 60, 0))                           # minute 60: neither
    groups.append(GE.group_10a(PI, PTY, "ROCK MUS", 0, ab=1))                       # the A/B flag flips: the old name goes
    groups.append(RG.group_2(PI, PTY, RT, 0))
    bits = RG.stream_bits(groups)
    for mb in (0, 2):
        dec, _, _ = run_pair(fmrx, bits, mb)
        x = fmrx.rds_station_ext_dict(dec.ext[0])
        assert x["ct"] == dict(mjd=0x1ABCD, hour=23, minute=59, offset_minutes=-60, bit_index=x["ct"]["bit_index"]), x
        cyc = GE.cycle_groups(RT)
        assert x["ct"]["bit_index"] == 104 * (2 * cyc - 3) and x["ct_count"] == 2
        assert (x["ecc"], x["lang"], x["pin"]) == (0xE0, 0x009, 0x5A21), x
        assert x["af"] == [88.1, 99.9, 107.9] and x["af_announced"] == 3, x
        assert (x["di"], x["di_mask"]) == (0b1001, 0xF), x
        assert (x["ptyn"], x["ptyn_mask"], x["ptyn_ab"]) == ("ROCK    ", 1, 1), x
        assert x["group_types"] == ["0A", "1A", "2A", "4A", "10A"], x
    # before the flip the name is whole; a stream without 4A / 10A has neither; version-B groups are named as such
    dec, _, _ = run_pair(fmrx, RG.stream_bits(GE.station_schedule(PI, PTY, PS, RT, 1, **STATION)), 0)
    x = fmrx.rds_station_ext_dict(dec.ext[0])
    assert (x["ptyn"], x["ptyn_mask"], x["ptyn_ab"]) == ("FOOTBALL", 3, 0)
    dec, _, _ = run_pair(fmrx, RG.stream_bits(RG.station_groups(PI, PTY, PS, RT, 12, version="B", rt_version="B")), 0)
    x = fmrx.rds_station_ext_dict(dec.ext[0])
    assert x["group_types"] == ["0B", "2B"] and x["ct"] is None and x["ecc"] is None and x["af"] == [] and x["ptyn_ab"] == 2
    # an invalid clock time alone: the group type is seen, the time is not taken
    dec, _, _ = run_pair(fmrx, RG.stream_bits([GE.group_4a(PI, PTY, 60000, 24, 0, 0)] * 4), 0)
    x = fmrx.rds_station_ext_dict(dec.ext[0])
    assert x["group_types"] == ["4A"] and x["ct"] is None and x["ct_count"] == 0


# ---- through the oracle's chain -------------------------------------------------------------------------------------------

def test_noisy_station_through_the_oracle_chain(fmrx):
    """2.4 s of a station (amplitude 0.05) with white noise of sigma 0.12 on the discriminator signal through the CPU oracle's
    RDS chain.  The level was picked on the model: with max_burst 0, 76 of 102 blocks pass (75 %), one sync loss; with
    max_burst 2, 95 of 104 (91 %), none (sigma 0.10: 94 % / 98 %; 0.14: 41 % / 74 %; 0.16: the PS no longer comes through)."""
    import rds_oracle as R
    x = RG.station_demod(int(240000 * 2.4), chip_offset=311.0, noise=0.12, amplitude=0.05)
    chain = R.RdsChain(upsamp=247, decim=960, sps=26)
    rows = [chain.process(x[i:i + 9600])["rrc_i"] for i in range(0, len(x) - 9600 + 1, 9600)]
    res = {}
    for mb in (0, 2):
        dec, model = fmrx.RdsStationDecoder(0, max_burst=mb), X.StationExtModel(26, mb)
        for k, row in enumerate(rows):
            _, g = dec.feed_rrc(row)
            rec, mg = model.feed_rrc(row)
            assert dec.record.tobytes() == rec and g.tobytes() == b"".join(mg) and dec.ext.tobytes() == model.ext_record(), (mb, k)
        res[mb] = fmrx.rds_station_dict(dec.record[0])
    print({mb: (s["good_blocks"], s["blocks"]) for mb, s in res.items()})
    assert 0.5 <= res[0]["good_blocks"] / res[0]["blocks"] <= 0.95, res[0]
    assert res[2]["good_blocks"] > res[0]["good_blocks"]
    assert (res[2]["pi"], res[2]["ps"]) == (0xC201, "TESTFM  "), res[2]


# ---- layout, interface, refusals ------------------------------------------------------------------------------------------

def test_ext_record_layout_matches_the_header(fmrx):
    hdr = open(os.path.join(ROOT, "include", "fmrx.h")).read()
    ctypes_of = {"uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "char": C.c_char}
    name, dt = "fmrx_rds_station_ext", fmrx.RDS_STATION_EXT_DTYPE
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
    sizes = [int(v) for v in re.findall(r"sizeof\(%s\) == (\d+)" % name, hdr)]
    assert sizes == [128, 128], "static asserts for C++ and C"
    assert C.sizeof(S) == dt.itemsize == 128
    assert [f[0] for f in fields] == list(dt.names)
    for f, t in fields:
        assert getattr(S, f).offset == dt.fields[f][1] and C.sizeof(t) == dt.fields[f][0].itemsize, f
    assert X.StationExtModel(26, 3).ext_record() == fmrx.RdsStationDecoder(0, max_burst=3).ext.tobytes()
    blank = np.frombuffer(X.StationExtModel(26, 0).ext_record(), dt)[0]
    assert bytes(blank["ptyn"]) == b" " * 8 and blank["ptyn_ab"] == 2
    assert not np.frombuffer(X.StationExtModel(26, 0).ext_record(), np.uint8)[list(range(76)) + list(range(84, 98)) + list(range(99, 128))].any()


def test_interface_and_refusals(fmrx):
    L, lib = fmrx.lib, C.CDLL(fmrx.LIB_PATH)
    for sym in ("fmrx_rds_station_set_correction", "fmrx_rds_station_ext_get", "fmrx_rds_block_correct",
                "fmrx_rds_bank_set_station_options", "fmrx_rds_bank_stations_ext"):
        assert hasattr(lib, sym), sym
    assert callable(fmrx.RdsBank.stations_ext) and callable(fmrx.rds_station_ext_dict)
    d = fmrx.RdsStationDecoder(0)
    x = np.zeros(1, fmrx.RDS_STATION_EXT_DTYPE)
    for mb in (-1, 6):
        assert L.fmrx_rds_station_set_correction(d._h, mb) == fmrx.EINVAL
        with pytest.raises(fmrx.FmrxError):
            fmrx.RdsStationDecoder(0, max_burst=mb)
    assert L.fmrx_rds_station_set_correction(None, 2) == fmrx.EINVAL
    assert L.fmrx_rds_station_ext_get(None, x.ctypes.data) == fmrx.EINVAL
    assert L.fmrx_rds_station_ext_get(d._h, None) == fmrx.EINVAL
    assert L.fmrx_rds_station_set_correction(d._h, 5) == fmrx.OK and d.ext[0]["max_burst"] == 5
    d.feed_bits([])                                                # nothing fed yet
    assert L.fmrx_rds_station_set_correction(d._h, 2) == fmrx.OK
    d.feed_bits(streams()["2-bit burst in every third block"][:1000])
    assert L.fmrx_rds_station_set_correction(d._h, 3) == fmrx.EINVAL          # after a feed
    assert d.ext[0]["max_burst"] == 2 and d.ext[0]["corrected_blocks"] > 0
    d.reset()
    assert d.ext.tobytes() == X.StationExtModel(26, 2).ext_record(), "reset clears the record and keeps the option"
    assert L.fmrx_rds_station_set_correction(d._h, 3) == fmrx.OK              # right after reset
    info, n = C.c_uint16(0), C.c_int(0)
    w = block_word(0x1234, 0)
    assert L.fmrx_rds_block_correct(w, 0, 2, None, None) == 0                  # info / burst_len are optional
    for args in ((w, -1, 2), (w, 5, 2), (w, 0, -1), (w, 0, 6), (1 << 26, 0, 2)):
        assert L.fmrx_rds_block_correct(*args, C.byref(info), C.byref(n)) == -1, args
    assert L.fmrx_rds_bank_set_station_options(None, 2, 1) == fmrx.EINVAL
    assert L.fmrx_rds_bank_stations_ext(None, x.ctypes.data) == fmrx.EINVAL


def test_standalone_program_under_sanitizers(tmp_path):
    """rds_station.hpp as a plain C++ program (tests/cpp/rds_station_ext_check.cpp) built with AddressSanitizer and
    UndefinedBehaviorSanitizer, every buffer a heap block of its exact size, on the streams above: no report, and the records
    it prints are the model's."""
    import subprocess
    exe = tmp_path / "rds_station_ext_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "software-defined-radio_amd", "csrc"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "rds_station_ext_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pieces = (0, 1, 25, 26, 27, 103, 190, 517)
    for name in ("2-bit burst across block boundaries", "5-bit bursts", "version B: errors in B and C'", "six failed blocks in a row",
                 "garbage in front"):
        bits = streams()[name]
        path = tmp_path / "bits"
        path.write_bytes(bytes(bits))
        for mb in (0, 2, 5):
            r = subprocess.run([str(exe), str(path), str(mb)], capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, (name, mb, r.stderr[-2000:])
            model, groups, at, k = X.StationExtModel(26, mb), [], 0, 0
            while at < len(bits):
                n = pieces[k % 8]
                groups += model.feed_bits(bits[at:at + n])[1]
                at, k = at + n, k + 1
            want = [f"group {g.hex()}" for g in groups] + [f"station {model.record().hex()}", f"ext {model.ext_record().hex()}",
                                                            f"groups {len(groups)}"]
            assert r.stdout.split("\n")[:-1] == want, (name, mb)
