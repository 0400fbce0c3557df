"""The signal meters on the device (fmrx_meters_*) against tests/_meters_model.py: the RF group's integers exactly, the MPX
group's float64 sums within bounds derived from the arithmetic, for rows of every alignment and pitch, past the 65 535th
channel, twice for determinism, and the API's edges."""
import functools

import numpy as np
import pytest

import _meters_model as mm

pytestmark = pytest.mark.gpu

IF_FS = 240000.0
RF_FIELDS, REL = mm.RF_FIELDS, mm.REL


@functools.lru_cache(maxsize=None)
def rows_and_model(n_channels, n_iq_bytes, n_if):
    rng = np.random.default_rng(1000 * n_channels + n_if)
    iq = rng.integers(0, 256, (n_channels, n_iq_bytes), dtype=np.uint8)
    iq[:, 1], iq[:, 6], iq[:, -1], iq[:, -4] = 0, 255, 0, 255          # both rails, at an I and a Q byte, whatever the length
    x = rng.uniform(-1.5, 1.5, (n_channels, n_if)).astype(np.float32)
    iq.setflags(write=False)
    x.setflags(write=False)
    want = np.array([mm.record(iq[c], x[c], IF_FS) for c in range(n_channels)])
    extra = [mm.mpx_group(x[c], IF_FS) for c in range(n_channels)]
    return iq, x, want, extra


def on_device(torch, rows, extra, offset, seed):
    """rows [N][n] -> a device tensor holding them at `offset` elements from its (aligned) start, pitch n + extra, random
    values in every gap; returns (tensor, address of row 0, pitch in elements)."""
    N, n = rows.shape
    pitch = n + extra
    rng = np.random.default_rng(seed)
    if rows.dtype == np.uint8:
        buf = rng.integers(0, 256, offset + N * pitch, dtype=np.uint8)
    else:
        buf = rng.uniform(-100.0, 100.0, offset + N * pitch).astype(np.float32)
    buf[offset:].reshape(N, pitch)[:, :n] = rows
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset * rows.dtype.itemsize, pitch


def check_rf(got, want, what):
    for f in RF_FIELDS:
        assert np.array_equal(got[f], want[f]), f"{what}: {f}: first difference at channel {int(np.argmax(got[f] != want[f]))}"


def check_mpx(got, want, extra, what):
    assert np.array_equal(got["n_if"], want["n_if"]) and np.array_equal(got["segments"], want["segments"]), what
    assert np.array_equal(got["max_abs"], want["max_abs"]), f"{what}: max_abs"
    for c in range(len(got)):
        e = extra[c]
        assert abs(got["sum_x"][c] - want["sum_x"][c]) <= REL * e["sum_abs"], f"{what}: sum_x, channel {c}"
        assert abs(got["sum_x2"][c] - want["sum_x2"][c]) <= REL * want["sum_x2"][c], f"{what}: sum_x2, channel {c}"
        d = np.abs(got["probe"][c] - want["probe"][c])
        assert np.all(d <= REL * e["bound"]), f"{what}: probe, channel {c}: {d} against {REL * e['bound']}"
        assert np.all(got["probe"][c][5:] == 0.0)


SHAPES = [(1, 64, 1024), (3, 2050, 1027), (65, 20480, 2048 + 5), (8, 192000, 9600)]


@pytest.mark.parametrize("base", [0, 1], ids=["aligned", "offset-3-bytes-1-float"])
@pytest.mark.parametrize("extra", [0, 16, 20])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_records_equal_the_model(fmrx, shape, extra, base):
    """Device rows at pitches of the row length + 0, 16, 20 (bytes / floats), from base addresses that are 16-byte aligned and
    that are 3 bytes / 1 float past it: the wide-load and the sample-by-sample paths of both passes."""
    import torch
    N, n_bytes, n_if = shape
    iq, x, want, extra_m = rows_and_model(*shape)
    t_iq, p_iq, pitch_iq = on_device(torch, iq, extra, 3 * base, 1)
    t_x, p_x, pitch_x = on_device(torch, x, extra, base, 2)
    m = fmrx.Meters(IF_FS, N)
    m.process_dev(p_iq, pitch_iq, n_bytes, p_x, pitch_x, n_if)
    got = m.collect()
    check_rf(got, want, f"{shape} pitch +{extra} base {base}")
    check_mpx(got, want, extra_m, f"{shape} pitch +{extra} base {base}")
    m.close()


def test_channels_past_the_grid_limit(fmrx):
    """66 000 channels of 64 bytes and 1024 floats: the channel rides in the grid's x.  Channels 0, 65 535, 65 536 and 65 999
    against the model; sum p of every channel against numpy."""
    import torch
    N, n_bytes, n_if = 66000, 64, 1024
    rng = np.random.default_rng(66)
    iq = rng.integers(0, 256, (N, n_bytes), dtype=np.uint8)
    x = rng.random((N, n_if), dtype=np.float32) * 3.0 - 1.5
    t_iq, t_x = torch.from_numpy(iq.copy()).cuda(), torch.from_numpy(x.copy()).cuda()
    m = fmrx.Meters(IF_FS, N)
    m.process_dev(t_iq.data_ptr(), n_bytes, n_bytes, t_x.data_ptr(), n_if, n_if)
    got = m.collect()
    pick = [0, 65535, 65536, 65999]
    want = np.array([mm.record(iq[c], x[c], IF_FS) for c in pick])
    check_rf(got[pick], want, "66 000 channels")
    check_mpx(got[pick], want, [mm.mpx_group(x[c], IF_FS) for c in pick], "66 000 channels")
    d = iq.astype(np.int64) - 128
    assert np.array_equal(got["m2"], (d * d).sum(axis=1).astype(np.uint64))
    assert np.array_equal(got["max_abs"], np.abs(x).max(axis=1).astype(np.float64))
    m.close()


def test_two_calls_give_the_same_bytes(fmrx):
    import torch
    shape = SHAPES[2]
    iq, x, want, _ = rows_and_model(*shape)
    t_iq, t_x = torch.from_numpy(iq.copy()).cuda(), torch.from_numpy(x.copy()).cuda()
    m = fmrx.Meters(IF_FS, shape[0])
    recs = []
    for _ in range(2):
        m.process_dev(t_iq.data_ptr(), shape[1], shape[1], t_x.data_ptr(), shape[2], shape[2])
        recs.append(m.collect().tobytes())
    assert recs[0] == recs[1]
    # a second call before collect replaces the results: other rows, then these again
    t_other = t_iq.flip(0).contiguous()
    m.process_dev(t_other.data_ptr(), shape[1], shape[1], t_x.data_ptr(), shape[2], shape[2])
    m.process_dev(t_iq.data_ptr(), shape[1], shape[1], t_x.data_ptr(), shape[2], shape[2])
    assert m.collect().tobytes() == recs[0]
    m.close()


def test_a_missing_input_reads_zero(fmrx):
    import torch
    shape = SHAPES[1]
    iq, x, want, extra_m = rows_and_model(*shape)
    t_iq, t_x = torch.from_numpy(iq.copy()).cuda(), torch.from_numpy(x.copy()).cuda()
    m = fmrx.Meters(IF_FS, shape[0])
    zero = np.zeros(shape[0], mm.METER_DTYPE)
    m.process_dev(None, 0, 0, t_x.data_ptr(), shape[2], shape[2])
    got = m.collect()
    for f in RF_FIELDS:
        assert np.array_equal(got[f], zero[f]), f
    check_mpx(got, want, extra_m, "no I/Q input")
    m.process_dev(t_iq.data_ptr(), shape[1], shape[1], None, 0, 0)
    got = m.collect()
    check_rf(got, want, "no demod input")
    for f in ("n_if", "segments", "sum_x", "sum_x2", "max_abs", "probe"):
        assert np.array_equal(got[f], zero[f]), f
    m.close()


def test_rejected_arguments(fmrx):
    import torch
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.Meters(100000.0, 1)
    assert e.value.code == fmrx.EINVAL
    t_x = torch.zeros(2048, dtype=torch.float32, device="cuda")
    t_iq = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    m = fmrx.Meters(IF_FS, 1)
    for args in [(None, 0, 0, t_x.data_ptr(), 1000, 1000),           # less than one segment
                 (t_iq.data_ptr(), 2048, 63, None, 0, 0),            # an odd byte count
                 (None, 0, 0, t_x.data_ptr() + 2, 1024, 1024)]:      # a row that is not a float's address
        with pytest.raises(fmrx.FmrxError) as e:
            m.process_dev(*args)
        assert e.value.code == fmrx.EINVAL
    m.close()


def test_host_rows_equal_device_rows(fmrx):
    import torch
    shape = SHAPES[1]
    iq, x, want, extra_m = rows_and_model(*shape)
    m = fmrx.Meters(IF_FS, shape[0])
    got = m.process(iq, x)
    check_rf(got, want, "host rows")
    check_mpx(got, want, extra_m, "host rows")
    t_iq, t_x = torch.from_numpy(iq.copy()).cuda(), torch.from_numpy(x.copy()).cuda()
    m.process_dev(t_iq.data_ptr(), shape[1], shape[1], t_x.data_ptr(), shape[2], shape[2])
    dev = m.collect()
    check_mpx(dev, want, extra_m, "device rows")
    # the staged host rows sit at 16-byte aligned pitches (one 16-byte load per thread and segment), these device rows at a
    # pitch of 1027 floats (four 4-byte loads): the same additions either way, so the same bytes, float64 sums included
    for f in mm.METER_DTYPE.names:
        assert np.array_equal(dev[f], got[f]), f
    assert dev.tobytes() == got.tobytes()
    # the derived levels of a record, through the handle
    lv, ref = m.derive(got[0]), mm.derive(want[0], IF_FS)
    assert all(abs(lv[k] - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])) for k in mm.LEVEL_NAMES)
    m.close()
