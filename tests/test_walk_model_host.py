"""The one-pole walk's order on the host (no GPU): tests/_walk_events.py -- the verify step as the device's workgroup runs it,
windows, strides, repair branches and all -- returns the bits, the state and the miss count of both filters' parallel_rows
and serial on every fixture of tests/test_gpu_onepole_walk.py (tests/_walk_cases.py), and those fixtures walk every branch
of it.  The GPU tests are only as strong as test_what_the_fixtures_exercise: it is what proves the branches are reached."""
import numpy as np
import pytest

import _deemph_model as m
import _highcut_cases as hcc
import _highcut_model as hm
import _walk_cases as wc
import _walk_events as we
from _fir_model import fmaf

F32 = np.float32
P75, B75 = m.design(wc.FS, 75.0)
SEVERAL = ("boundary_equal", "miss_on_stride", "miss_in_later_window", "chain_over_window")   # in two (shape, input) cases at least


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_scalar_fmaf_equals_the_array_one():
    """fmaf1 on random triples of every magnitude, on the subnormal range, on infinities and NaN, and on sums that land on a
    float32 midpoint in float64 which the exact value misses (the double-rounding cases of tests/test_fir_model_host.py)"""
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(6000) * 10.0 ** rng.integers(-20, 20, 6000)).astype(F32)
    b = (rng.standard_normal(6000) * 10.0 ** rng.integers(-20, 20, 6000)).astype(F32)
    c = (rng.standard_normal(6000) * 10.0 ** rng.integers(-40, 38, 6000)).astype(F32)
    tiny = (rng.standard_normal(2000) * 2e-38).astype(F32)
    a, b, c = np.concatenate([a, np.full(2000, 0.75, F32)]), np.concatenate([b, tiny]), np.concatenate([c, tiny[::-1]])
    one_p, one_m = F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23)
    extra = [(np.inf, 0.5, 1.0), (np.inf, 0.5, -np.inf), (0.5, np.nan, 1.0), (0.0, -1.0, 0.0), (-0.0, 1.0, -0.0), (3e38, 3.0, 1.0)]
    for k in (-100, -20, 0, 20, 100):
        s = 2.0 ** k
        extra.append((one_p, F32(one_m * 2.0 ** -24 * s), F32((1 + 2.0 ** -23) * s)))
        extra.append((-one_p, F32(one_m * 2.0 ** -24 * s), F32((1 + 2.0 ** -22 + 2.0 ** -23) * s)))
    a, b, c = (np.concatenate([v, np.array([t[i] for t in extra], F32)]) for i, v in enumerate((a, b, c)))
    with np.errstate(all="ignore"):
        want = fmaf(a, b, c)
        got = np.array([we.fmaf1(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)]).astype(F32)
    assert we.same(got, want).all()
    assert [we.same1(x, y) for x, y in ((0.0, -0.0), (0.0, 0.0), (np.nan, np.nan), (1.0, np.nan), (np.inf, np.inf))] == [False, True, True, False, True]


@pytest.fixture(scope="module")
def sweep():
    """shape -> the de-emphasis cases of every length, computed once"""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = [wc.deemph_case(*shape, n, P75, B75) for _, n in wc.lengths(shape[1])]
        return cache[shape]
    return get


def check_against_serial(cases, p, b0):
    """One serial walk for all of the cases' rows side by side (zeros behind a shorter row: a row's first n outputs do not
    depend on them): the parallel walk's bits and state, row for row"""
    n_max = max(c["n"] for c in cases)
    x = np.concatenate([np.pad(c["x"], ((0, 0), (0, n_max - c["n"]))) for c in cases])
    ys, _ = m.serial(x, p, b0, np.concatenate([c["state"] for c in cases]))
    at = 0
    for c in cases:
        rows, n = c["x"].shape
        tag = (c["W"], c["L"], n)
        assert m.same(c["y"], ys[at:at + rows, :n]).all(), tag
        assert m.same(c["state_out"], np.stack([c["x"][:, -1], ys[at:at + rows, n - 1]], axis=1)).all(), tag
        at += rows


def check_device_order(c):
    R = len(c["dev_y"])
    tag = (c["W"], c["L"], c["n"])
    assert m.same(c["dev_y"], c["y"][:R]).all(), tag
    assert m.same(c["dev_state"], c["state_out"][:R]).all(), tag
    assert [e["miss"] for e in c["events"]] == c["missed"][:R].tolist(), tag
    for k, e in zip(c["kinds"], c["events"]):
        assert k not in wc.QUIET or e["miss"] == 0, (tag, k)


@pytest.mark.parametrize("shape", wc.SHAPES, ids=wc.shape_id)
def test_deemph_parallel_serial_and_the_device_order_agree(sweep, shape):
    """every length of the sweep, a carried non-zero state on the rows that can have one: parallel == serial in bits and state,
    the device's order == parallel in bits, state and misses per row; a row of zeros or subnormals misses nothing"""
    cases = sweep(shape)
    assert any(np.any(c["state"] != 0) for c in cases)
    check_against_serial(cases, P75, B75)
    for c in cases:
        check_device_order(c)
    print(f"{wc.shape_id(shape)}: {len(cases)} lengths, {we.table(we.total(e for c in cases for e in c['events']))}")


@pytest.mark.parametrize("shape", [(0, 4), (33, 31), (256, 1)], ids=wc.shape_id)
def test_deemph_at_50_us(shape):
    p, b0 = m.design(wc.FS, 50.0)
    cases = [wc.deemph_case(*shape, n, p, b0) for s, n in wc.lengths(shape[1]) if s in (2, 65, 1025)]
    check_against_serial(cases, p, b0)
    for c in cases:
        check_device_order(c)


def test_what_the_fixtures_exercise(sweep):
    """Over the de-emphasis sweep every event of _walk_events occurs, and the boundary-equal branch, a miss on a lane's later
    stride, a miss in a window that `from = hi` entered and a repair that resumes behind its window each in several (shape,
    input) cases.  The window-edge rows put their first miss where they aim it; the late Inf/NaN chain starts in the second
    window and ends at the row's end."""
    total, where = dict.fromkeys(we.EVENTS, 0), {k: set() for k in we.EVENTS}
    print()
    for shape in wc.SHAPES:
        sub = dict.fromkeys(we.EVENTS, 0)
        for c in sweep(shape):
            for kind, ev, found in zip(c["kinds"], c["events"], c["found"]):
                for k in we.EVENTS:
                    sub[k] += ev[k]
                    if ev[k]:
                        where[k].add((shape, kind))
                if c["nseg"] >= wc.LONG and kind.startswith("edge"):
                    frm, hi, fm, resume = found[0]
                    aim = wc.edge_seams(*shape, c["nseg"])[kind]
                    assert fm == aim, (shape, c["n"], kind, found[0])
                    if kind == "edge: last seam":
                        assert (frm, hi, aim) == (1, 8193, 8192) and ev["miss_at_last_seam"] >= 1
                        assert c["nseg"] == 8193 or resume > hi
                    if kind == "edge: first seam" and c["nseg"] > 8193:
                        assert (frm, aim) == (8193, 8193) and ev["miss_in_later_window"] == 1 and ev["miss_at_first_seam"] >= 1
                    if kind == "edge: chain across" and c["nseg"] > 8193:
                        assert frm == 1 and aim < 8192 and resume > hi == 8193 and ev["chain_over_window"] >= 1
                if c["nseg"] == 16390 and kind == "late Inf/NaN":
                    first = found[0]
                    assert first[2] > 8193 and first[0] == 8193 and ev["miss_in_later_window"] >= 1, (shape, first)
                    assert found[-1][3] == c["nseg"] and ev["row_end"] == 1, (shape, found[-1])
        print(f"{wc.shape_id(shape):>8}: {we.table(sub)}")
        for k in we.EVENTS:
            total[k] += sub[k]
    print(f"{'all':>8}: {we.table(total)}")
    for k in we.EVENTS:
        print(f"{k}: {len(where[k])} (shape, input) cases")
        assert total[k] >= 1, k
    for k in SEVERAL:
        assert len(where[k]) >= 2, (k, where[k])
        assert len({s for s, _ in where[k]}) >= 2 and len({i for _, i in where[k]}) >= 2, (k, where[k])
    assert any(i.startswith("flush") for _, i in where["boundary_equal"])


@pytest.fixture(scope="module")
def three_long_cases():
    out = []
    for shape, nseg in (((8, 2), 16390), ((256, 1), 8194), ((0, 4), 8194)):
        n = [n for s, n in wc.lengths(shape[1]) if s == nseg][-1]
        out.append((shape, n, wc.deemph_case(*shape, n, P75, B75)))
    return out


@pytest.mark.parametrize("drop", we.DROPS)
def test_a_walk_without_one_of_its_lines_is_noticed(three_long_cases, drop):
    """_walk_events.verify with one line taken out -- the u-stride term of the scan, `from = hi`, the boundary-equal branch, the
    rewrite of the last segment's end at the row's end -- computes something else than the model on rows of the sweep: other
    bits, another state or another miss count.  A device with that mistake fails tests/test_gpu_onepole_walk.py on them."""
    seen = []
    for shape, n, c in three_long_cases:
        y, st, evs, _ = wc.device_order(c["x"], c["state"], c["spec"], P75, B75, shape[1], drop=(drop,))
        for r, kind in enumerate(c["kinds"]):
            what = [w for w, bad in (("bits", not m.same(y[r], c["y"][r]).all()), ("state", not m.same(st[r], c["state_out"][r]).all()),
                                     ("misses", evs[r]["miss"] != c["missed"][r])) if bad]
            if what:
                seen.append((shape, n, kind, what))
    print(f"without {drop}:", *seen, sep="\n    ")
    assert len({(s, k) for s, _, k, _ in seen}) >= 2, drop


# ---- the high-cut ------------------------------------------------------------------------------------------------------------
def test_highcut_parallel_serial_and_the_device_order_agree():
    """The GPU test's high-cut cases, six calls each, the filter state carried: the pole moves within a call, comes down to 0
    inside one (the select takes over in mid-row) and reaches p_max.  Per call one serial walk for all cases' rows side by side."""
    cases = wc.highcut_cases()
    assert {(c["N"], c["ac"]) for c in cases} == {(N, ac) for N in (1, 3, 35) for ac in (1, 2)}
    assert {c["nseg"] for c in cases} == {65, 1025, 8194} and {(c["W"], c["L"]) for c in cases} == set(wc.SHAPES)
    models = []
    for c in cases:
        p = hm.params(**hcc.PSETS["fast"])
        p.update(warmup=c["W"], segment=c["L"])
        ctl = hm.control(p, hcc.IF_FS, hcc.AUDIO_FS)
        models.append((ctl, hcc.records(ctl, c["N"]), wc.HighcutWalk(ctl, c["N"], c["ac"], (c["W"], c["L"]))))
    p_max = models[0][0]["p_max"]
    n_max = max(c["n"] for c in cases)
    total, moved = dict.fromkeys(we.EVENTS, 0), set()
    for k in range(hcc.CALLS):
        xs, Ps, ys0 = [], [], []
        for c, (ctl, recs, mdl) in zip(cases, models):
            mdl.call(recs[k], wc.highcut_inputs(c, k)[0])
            l = mdl.last
            R = len(l["dev_y"])
            tag = (wc.highcut_id(c), k)
            assert hm.same(l["dev_y"], l["y"][:R]).all() and hm.same(l["dev_state"], l["state"][:R]).all(), tag
            assert [e["miss"] for e in l["events"]] == l["missed"][:R].tolist(), tag
            for e in l["events"]:
                for name in we.EVENTS:
                    total[name] += e[name]
            P = hm.poles(l["p0"], l["p1"], c["n"], p_max)
            moved |= {"moves"} if np.any(P[:, 0] != P[:, -1]) else set()
            moved |= {"comes down to 0 inside a call"} if np.any((P[:, 0] > 0) & (P[:, -1] == 0)) else set()
            moved |= {"p_max"} if np.any(P == p_max) else set()
            xs.append(np.pad(l["x"], ((0, 0), (0, n_max - c["n"]))))
            Ps.append(np.pad(P, ((0, 0), (0, n_max - c["n"]))))
            ys0.append(l["state_in"])
        x, P, yp = np.concatenate(xs), np.concatenate(Ps), np.concatenate(ys0).astype(F32)
        ys = np.zeros_like(x)
        for i in range(n_max):                                   # hm.serial's walk, on poles that every case computed for its own n
            yp = hm.filt(x[:, i], P[:, i], yp)
            ys[:, i] = yp
        at = 0
        for c, (_, _, mdl) in zip(cases, models):
            rows, n = mdl.last["x"].shape
            assert hm.same(mdl.last["y"], ys[at:at + rows, :n]).all() and hm.same(mdl.last["state"], ys[at:at + rows, n - 1]).all(), (wc.highcut_id(c), k)
            at += rows
    print(f"high-cut, {len(cases)} cases x {hcc.CALLS} calls: {we.table(total)}")
    assert moved == {"moves", "comes down to 0 inside a call", "p_max"}, moved
    assert total["miss"] > 0 and total["miss_on_stride"] > 0 and total["miss_in_later_window"] > 0


def test_highcut_serial_by_columns_is_hm_serial():
    """(the walk above is hm.serial's: one small case through both)"""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 50)).astype(F32)
    p0, p1, p_max = np.array([0, 0.7, 0.3], F32), np.array([0.7, 0, 0.3], F32), F32(0.72)
    want, _ = hm.serial(x, p0, p1, p_max)
    P, yp = hm.poles(p0, p1, 50, p_max), np.zeros(3, F32)
    for i in range(50):
        yp = hm.filt(x[:, i], P[:, i], yp)
        assert (bits(yp) == bits(want[:, i])).all()
