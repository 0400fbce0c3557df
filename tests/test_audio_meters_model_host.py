"""The audio meters without a GPU (include/fmrx.h: fmrx_audio_meters_*, fmrx_loudness_*): the design
against the table of ITU-R BS.1770-4 and against the model, the host walk against the model bit for bit, the standard's
readings, the gated integrator against a brute-force gating, the edge rules of the levels, and the exported symbols."""
import math
import re

import numpy as np
import pytest

import _audio_meters_model as am

RATES = (32000.0, 44100.0, 48000.0, 47999.0, 22051.5)
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
TABLE = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                  [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


def test_1_the_design_at_48_kHz_equals_the_standards_table(fmrx):
    for got in (am.design(48000.0), fmrx.audioMetersDesign(48000.0)):
        err = np.abs(got - TABLE).max()
        print(f"design at 48 kHz against the table: {err:.3e}")
        assert err <= 1e-12
    assert am.VH == 10.0 ** (3.999843853973347 / 20.0) and am.VB == am.VH ** 0.4996667741545416


@pytest.mark.parametrize("Fs", RATES)
def test_2_the_design_equals_the_model_bit_for_bit(fmrx, Fs):
    assert fmrx.audioMetersDesign(Fs).tobytes() == am.design(Fs).tobytes()
    assert fmrx.audioMetersBinLen(Fs) == am.bin_len(Fs) == int(Fs / 10 + 0.5)
    assert fmrx.lib.fmrx_audio_meters_max_bins(Fs, 10007) == am.max_bins(Fs, 10007)


def test_2_a_rate_out_of_range_is_refused(fmrx):
    for Fs in (0.0, -48000.0, 7999.0, 1e6, float("nan"), float("inf")):
        with pytest.raises(fmrx.FmrxError) as e:
            fmrx.audioMetersDesign(Fs)
        assert e.value.code == fmrx.EINVAL
        assert fmrx.audioMetersBinLen(Fs) == 0


def host_walk(fmrx, Fs, rows, states):
    """fmrx_audio_meters_walk channel by channel, in the model's shapes"""
    N, ac, n = rows.shape
    nb = am.max_bins(Fs, n)
    rec, bins = np.zeros(N, fmrx.AUDIO_METER_DTYPE), np.zeros((N, 2, nb))
    for c in range(N):
        rec[c], bins[c], states[c] = fmrx.audioMetersWalk(Fs, rows[c], states[c])
    return rec, bins


def state_of(states):
    return dict(z=np.stack([s["z"] for s in states]), bin_acc=np.stack([s["bin_acc"] for s in states]),
                bin_fill=np.array([int(s["bin_fill"]) for s in states], np.int64))


L48 = am.bin_len(48000.0)
# n of three calls each: 1, 7, bin_len, bin_len + 1, and lengths that leave a bin open across two calls (3000 + 1000 < 4800 <
# 3000 + 1000 + 900)
LENGTHS = {"1": (1, 1, 1), "7": (7, 7, 7), "bin_len": (L48, L48, L48), "bin_len + 1": (L48 + 1, L48 + 1, L48 + 1), "open bin": (3000, 1000, 900)}


@pytest.mark.parametrize("ac", [1, 2])
@pytest.mark.parametrize("name", list(LENGTHS))
def test_3_the_host_walk_equals_the_model_bit_for_bit(fmrx, ac, name):
    Fs, N = 48000.0, 5
    assert fmrx.AUDIO_METER_DTYPE == am.AUDIO_METER_DTYPE
    rng = np.random.default_rng(17 * ac + len(name))
    model, states = am.fresh(N), [None] * N
    done = 0
    for n in LENGTHS[name]:
        x = am.special_rows(rng, N, ac, n)
        want_rec, want_bins, model = am.walk(Fs, x, model)
        rec, bins = host_walk(fmrx, Fs, x, states)
        assert am.same(rec, want_rec), (name, n)
        assert am.same(bins, want_bins), (name, n)
        st = state_of(states)
        assert am.same(st["z"], model["z"]) and am.same(st["bin_acc"], model["bin_acc"]) and np.array_equal(st["bin_fill"], model["bin_fill"])
        done += int(rec["bins_done"][0])
        assert np.all(rec["bins_done"] == rec["bins_done"][0]) and rec["bins_done"][0] <= n // L48 + 1
    assert done == sum(LENGTHS[name]) // L48
    if name == "open bin":
        assert done == 1 and int(states[0]["bin_fill"]) == 100
    if name != "1":                          # the special rows did what they are there for
        assert np.isnan(want_rec["sum_k2"][-2, 0]) and np.isinf(want_rec["peak"][-1, ac - 1]) and np.isnan(want_rec["sum_k2"][-1, ac - 1])
        assert np.isfinite(want_rec["sum_k2"][:3]).all() and (n < 900 or want_rec["over"][:3, :ac].min() > 0)


def test_3_mono_fills_index_0_only_and_records_add(fmrx):
    rng = np.random.default_rng(3)
    x = (0.5 * rng.standard_normal((1, 6000))).astype(np.float32)
    a, bins_a, st = fmrx.audioMetersWalk(48000.0, x[:, :2500])
    b, bins_b, st = fmrx.audioMetersWalk(48000.0, x[:, 2500:], st)
    for r in (a, b):
        for f in ("over", "peak", "sum_x", "sum_x2", "sum_k2"):
            assert r[f][1] == 0
        assert r["sum_lr"] == 0
    assert np.all(bins_a[1] == 0) and np.all(bins_b[1] == 0)
    whole, bins_w, _ = fmrx.audioMetersWalk(48000.0, x)
    s = am.add(a, b)
    assert s["n"] == 6000 and s["bins_done"] == whole["bins_done"] == 1 and s["peak"][0] == whole["peak"][0] and s["over"][0] == whole["over"][0]
    assert bins_b[0, 0] == bins_w[0, 0]                                  # a bin that straddles the calls has the one-call walk's bits
    assert abs(s["sum_k2"][0] - whole["sum_k2"][0]) <= 1e-12 * whole["sum_k2"][0]


def test_3_too_few_bins_are_refused(fmrx):
    x = np.zeros((1, 4800), np.float32)
    rec, st, bins = np.zeros(1, fmrx.AUDIO_METER_DTYPE), np.zeros(1, fmrx.AUDIO_METER_STATE_DTYPE), np.zeros((2, 1))
    rc = fmrx.lib.fmrx_audio_meters_walk(48000.0, 1, x.ctypes.data, 4800, 4800, st.ctypes.data, rec.ctypes.data, bins.ctypes.data, 1)
    assert rc == fmrx.EINVAL


def sine(f, amp, Fs, n):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(n) / Fs)).astype(np.float32)


def test_4_a_full_scale_997_Hz_sine_in_one_row_reads_minus_3_01_LKFS(fmrx):
    Fs = 48000.0
    x = np.stack([sine(997.0, fmrx.AUDIO_FULL_SCALE, Fs, 48000), np.zeros(48000, np.float32)])
    rec, _, _ = fmrx.audioMetersWalk(Fs, x)
    got = fmrx.audioMetersDerive(rec, 2)["loudness_lkfs"]
    print(f"997 Hz at full scale, one row, 1 s: {got:.4f} LKFS")
    assert abs(got - -3.01) <= 0.01


@pytest.mark.parametrize("Fs,computed", [(48000.0, -22.993), (44100.0, -22.991), (32000.0, -22.979)])
def test_4_a_1_kHz_sine_at_minus_23_dBFS_in_both_rows_reads_minus_23_LKFS(fmrx, Fs, computed):
    n = int(Fs)
    s = sine(1000.0, fmrx.AUDIO_FULL_SCALE * 10.0 ** (-23.0 / 20.0), Fs, n)
    rec, _, _ = fmrx.audioMetersWalk(Fs, np.stack([s, s]))
    lv = fmrx.audioMetersDerive(rec, 2)
    print(f"1 kHz at -23 dBFS, both rows, 1 s at {Fs:.0f} Hz: {lv['loudness_lkfs']:.4f} LKFS")
    assert abs(lv["loudness_lkfs"] - -23.0) <= 0.1                      # EBU Tech 3341's tolerance
    assert abs(lv["loudness_lkfs"] - computed) <= 0.002
    assert abs(lv["correlation"] - 1.0) <= 1e-12 and lv["balance_db"] == 0.0 and abs(lv["peak_dbfs"][0] - -23.0) <= 0.01
    assert abs(lv["rms_dbfs"][0] - -26.01) <= 0.01


# ---- the integrator -----------------------------------------------------------------------------------------------------
FS, BIN = 48000.0, 4800


def energy(lufs):
    """a bin's sum y^2 of one row at a steady loudness"""
    return BIN * am.FULL_SCALE ** 2 * 10.0 ** ((lufs + 0.691) / 10.0)


def programme(parts):
    return np.concatenate([np.full(int(round(sec * 10)), energy(l)) for l, sec in parts])


def brute_force(e):
    """BS.1770-4's gating over every block of 4 bins, written out with logarithms"""
    z = np.array([e[j:j + 4].sum() for j in range(len(e) - 3)]) / (4 * BIN) / am.FULL_SCALE ** 2
    l = -0.691 + 10.0 * np.log10(np.maximum(z, 1e-300))
    ga = z[l > -70.0]
    if not len(ga):
        return -99.0
    gate = -0.691 + 10.0 * math.log10(ga.mean()) - 10.0
    return -0.691 + 10.0 * math.log10(z[(l > -70.0) & (l > gate)].mean())


def integrate(fmrx, e, per_push=7, max_blocks=36000, channels=2):
    """the bins e of channel 1 (row L and R half each) through fmrx_loudness_push in pushes of up to per_push bins; channel 0 silent"""
    loud = fmrx.Loudness(channels, BIN, max_blocks)
    for i in range(0, len(e), per_push):
        part = e[i:i + per_push]
        recs, bins = np.zeros(channels, fmrx.AUDIO_METER_DTYPE), np.zeros((channels, 2, per_push))
        recs["bins_done"][1] = len(part)
        bins[1, 0, :len(part)] = 0.25 * part
        bins[1, 1, :len(part)] = 0.75 * part
        loud.push(recs, bins)
    out = [loud.read(c) for c in range(channels)]
    loud.close()
    return out


@pytest.mark.parametrize("parts,computed", [
    ([(-36.0, 10), (-23.0, 60), (-36.0, 10)], -23.02),
    ([(-72.0, 10), (-36.0, 10), (-23.0, 60), (-36.0, 10), (-72.0, 10)], -23.02),
    ([(-26.0, 20), (-20.0, 20.1), (-26.0, 20)], -22.99)])
def test_5_the_integrator_against_a_brute_force_gating(fmrx, parts, computed):
    e = programme(parts)
    silent, got = integrate(fmrx, e)
    want, model = brute_force(e), am.gated(e, FS)
    print(f"{parts}: integrated {got['integrated']:.4f} LKFS, brute force {want:.4f}, model {model['integrated']:.4f}")
    assert abs(got["integrated"] - -23.0) <= 0.1
    assert abs(got["integrated"] - computed) <= 0.01
    assert abs(got["integrated"] - want) <= 1e-9 and abs(model["integrated"] - want) <= 1e-9
    assert got["blocks"] == model["blocks"] == len(e) - 3 and not got["full"]
    assert abs(got["momentary"] - parts[-1][0]) <= 1e-9 and abs(got["short_term"] - parts[-1][0]) <= 1e-9
    assert abs(model["momentary"] - got["momentary"]) <= 1e-9 and abs(model["short_term"] - got["short_term"]) <= 1e-9
    assert silent == dict(momentary=-99.0, short_term=-99.0, integrated=-99.0, blocks=0, full=False)


def test_5_the_gate_in_front_and_behind_changes_nothing(fmrx):
    a = integrate(fmrx, programme([(-36.0, 10), (-23.0, 60), (-36.0, 10)]))[1]["integrated"]
    b = integrate(fmrx, programme([(-72.0, 10), (-36.0, 10), (-23.0, 60), (-36.0, 10), (-72.0, 10)]))[1]["integrated"]
    assert abs(a - b) <= 1e-9


def test_5_silence_reads_minus_99(fmrx):
    for e in (np.zeros(100), np.full(100, energy(-80.0))):          # digital silence, and a noise floor under the absolute gate
        got = integrate(fmrx, e)[1]
        assert got["integrated"] == -99.0 and got["blocks"] == 97
        assert am.gated(e, FS)["integrated"] == -99.0
    assert integrate(fmrx, np.zeros(100))[1]["momentary"] == -99.0
    assert integrate(fmrx, np.full(3, energy(-20.0)))[1] == dict(momentary=-99.0, short_term=-99.0, integrated=-99.0, blocks=0, full=False)


def test_5_full_is_set_at_max_blocks_and_nothing_is_overwritten(fmrx):
    e = programme([(-23.0, 5), (-10.0, 5)])
    got = integrate(fmrx, e, max_blocks=40)[1]
    model = am.gated(e, FS, max_blocks=40)
    assert got["full"] and got["blocks"] == 40 and model["full"] and model["blocks"] == 40
    assert abs(got["integrated"] - -23.0) <= 1e-9 and abs(model["integrated"] - -23.0) <= 1e-9      # the loud end was not stored
    assert abs(got["momentary"] - -10.0) <= 1e-9                                                    # the running readings go on
    assert not integrate(fmrx, e[:42], max_blocks=40)[1]["full"] and integrate(fmrx, e[:43], max_blocks=40)[1]["full"]


def test_5_reset_clears_one_channel(fmrx):
    loud = fmrx.Loudness(2, BIN, 100)
    recs, bins = np.zeros(2, fmrx.AUDIO_METER_DTYPE), np.full((2, 2, 8), energy(-20.0) / 2)
    recs["bins_done"] = 8
    loud.push(recs, bins)
    loud.reset(0)
    assert loud.read(0)["blocks"] == 0 and loud.read(0)["integrated"] == -99.0
    assert loud.read(1)["blocks"] == 5 and abs(loud.read(1)["integrated"] - -20.0) <= 1e-9
    recs["bins_done"] = 9
    with pytest.raises(fmrx.FmrxError):
        loud.push(recs, bins)
    loud.close()


# ---- the levels ---------------------------------------------------------------------------------------------------------
def record(**kw):
    r = np.zeros((), am.AUDIO_METER_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def levels(fmrx, rec, ac, fs=2.0):
    got, want = fmrx.audioMetersDerive(rec, ac, fs), am.derive(rec, ac, fs)
    flat = dict(peak_dbfs_l=got["peak_dbfs"][0], peak_dbfs_r=got["peak_dbfs"][1], rms_dbfs_l=got["rms_dbfs"][0], rms_dbfs_r=got["rms_dbfs"][1],
                dc_l=got["dc"][0], dc_r=got["dc"][1], **{k: got[k] for k in ("loudness_lkfs", "correlation", "balance_db", "over_fraction")})
    assert set(flat) == set(am.AUDIO_LEVELS_NAMES)
    for k in flat:
        assert flat[k] == want[k] or abs(flat[k] - want[k]) <= 1e-12 * abs(want[k]), (k, flat[k], want[k])
    return flat


def test_6_the_levels_of_an_ordinary_record(fmrx):
    rng = np.random.default_rng(6)
    x = (0.4 * rng.standard_normal((2, 9000))).astype(np.float32)
    x[1] = 0.5 * x[0] + 0.1 * x[1]
    rec, _, _ = fmrx.audioMetersWalk(48000.0, x)
    lv = levels(fmrx, rec, 2)
    d = x.astype(np.float64)
    assert abs(lv["rms_dbfs_l"] - 10 * np.log10((d[0] ** 2).mean() / 4.0)) <= 1e-9
    assert abs(lv["peak_dbfs_r"] - 20 * np.log10(np.abs(d[1]).max() / 2.0)) <= 1e-9
    assert abs(lv["dc_l"] - d[0].mean()) <= 1e-12
    assert abs(lv["correlation"] - (d[0] * d[1]).sum() / np.sqrt((d[0] ** 2).sum() * (d[1] ** 2).sum())) <= 1e-12 and 0.9 < lv["correlation"] < 1.0
    assert abs(lv["balance_db"] - 10 * np.log10((d[0] ** 2).sum() / (d[1] ** 2).sum())) <= 1e-9
    assert lv["over_fraction"] == 0.0
    assert levels(fmrx, rec, 2, fs=1.0)["rms_dbfs_l"] == pytest.approx(lv["rms_dbfs_l"] + 20 * np.log10(2.0), abs=1e-9)


def test_6_edge_rules(fmrx):
    zero = levels(fmrx, record(), 2)                                             # n = 0: every dB value -99, everything else 0
    assert zero == dict(peak_dbfs_l=-99.0, peak_dbfs_r=-99.0, rms_dbfs_l=-99.0, rms_dbfs_r=-99.0, dc_l=0.0, dc_r=0.0, loudness_lkfs=-99.0,
                        correlation=0.0, balance_db=-99.0, over_fraction=0.0)
    silent = levels(fmrx, record(n=1920), 2)                                     # dead air
    assert silent == zero
    one = record(n=100, peak=(1.0, 0.0), sum_x=(5.0, 0.0), sum_x2=(50.0, 0.0), sum_k2=(50.0, 0.0), over=(3, 1))
    lv = levels(fmrx, one, 2)                                                    # the right row is missing
    assert lv["balance_db"] == 99.0 and lv["correlation"] == 0.0 and lv["rms_dbfs_r"] == -99.0 and lv["peak_dbfs_r"] == -99.0
    assert lv["dc_l"] == 0.05 and lv["over_fraction"] == 0.02
    flipped = levels(fmrx, record(n=100, sum_x2=(0.0, 50.0), sum_k2=(0.0, 50.0)), 2)
    assert flipped["balance_db"] == -99.0
    mono = levels(fmrx, one, 1)                                                  # mono: no image; over over n samples
    assert mono["balance_db"] == 0.0 and mono["correlation"] == 0.0 and mono["over_fraction"] == 0.04
    huge = levels(fmrx, record(n=1, peak=(1e30, 1e30), sum_x2=(1e300, 1e-300), sum_k2=(1e300, 0.0)), 2)
    assert huge["peak_dbfs_l"] == 99.0 and huge["rms_dbfs_l"] == 99.0 and huge["loudness_lkfs"] == 99.0 and huge["balance_db"] == 99.0
    tiny = levels(fmrx, record(n=1, peak=(1e-30, 0.0), sum_x2=(1e-300, 1e300), sum_k2=(1e-300, 0.0)), 2)
    assert tiny["peak_dbfs_l"] == -99.0 and tiny["rms_dbfs_l"] == -99.0 and tiny["loudness_lkfs"] == -99.0 and tiny["balance_db"] == -99.0
    nan = levels(fmrx, record(n=10, peak=(np.inf, 1.0), sum_x2=(np.nan, 1.0), sum_k2=(np.nan, 1.0), sum_lr=np.nan), 2)
    assert nan["rms_dbfs_l"] == -99.0 and nan["loudness_lkfs"] == -99.0 and nan["peak_dbfs_l"] == 99.0 and nan["correlation"] == 0.0
    anti = levels(fmrx, record(n=10, peak=(1.0, 1.0), sum_x2=(10.0, 10.0), sum_k2=(10.0, 10.0), sum_lr=-10.0), 2)
    assert anti["correlation"] == -1.0 and anti["balance_db"] == 0.0              # out of phase
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(fmrx.FmrxError):
            fmrx.audioMetersDerive(record(), 2, bad)
    with pytest.raises(fmrx.FmrxError):
        fmrx.audioMetersDerive(record(), 3)


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_7_every_new_symbol_is_exported_and_mirrored(fmrx):
    with open(fmrx.HEADER_PATH) as f:
        declared = set(re.findall(r"FMRX_API\s+[\w\s\*]+?\b(fmrx_(?:audio_meters|loudness)_\w+)\s*\(", f.read()))
    assert declared == {"fmrx_audio_meters_design", "fmrx_audio_meters_bin_len", "fmrx_audio_meters_max_bins", "fmrx_audio_meters_walk",
                        "fmrx_audio_meters_derive", "fmrx_audio_meters_create", "fmrx_audio_meters_destroy", "fmrx_audio_meters_reset",
                        "fmrx_audio_meters_state_get",
                        "fmrx_audio_meters_process_dev", "fmrx_audio_meters_collect", "fmrx_audio_meters_process", "fmrx_loudness_create",
                        "fmrx_loudness_destroy", "fmrx_loudness_reset", "fmrx_loudness_push", "fmrx_loudness_read"}
    for name in declared:
        assert hasattr(fmrx.lib, name), name
    for name in ("AudioMeters", "audioMetersDesign", "audioMetersDerive", "audioMetersWalk", "audioMetersBinLen", "Loudness", "AUDIO_METER_DTYPE",
                 "AUDIO_LEVELS_DTYPE", "AUDIO_METER_STATE_DTYPE", "LOUDNESS_LEVELS_DTYPE"):
        assert hasattr(fmrx, name), name
    for name in ("for_bank", "process_bank", "process_dev", "process", "collect", "state", "reset", "close", "derive"):
        assert hasattr(fmrx.AudioMeters, name), name
    for name in ("for_meters", "push", "read", "reset", "close"):
        assert hasattr(fmrx.Loudness, name), name
    assert fmrx.AUDIO_METER_DTYPE.itemsize == 104 and fmrx.AUDIO_LEVELS_DTYPE.itemsize == 80
