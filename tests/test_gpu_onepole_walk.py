"""The one-pole walk (csrc/onepole_walk.hpp) on the device beyond what the stages' own tests reach: rows of up to 16 390 segments
-- verify workgroups of 1024 lanes, seams on a lane's later strides, a second and a third window -- every repair branch, and
lane shapes with W > L, W = 0, L = 1, W + L off the 32-step batch and the hand-over in a later batch.  Everything is bit for bit
against the filters' models (any NaN equals any NaN); miss counts and diagnostics equal the models'.  The fixtures are those
of tests/_walk_cases.py; tests/test_walk_model_host.py shows which branches of the verify step they walk
(test_what_the_fixtures_exercise), and every test here prints the events of its own rows (tests/_walk_events.py)."""
import importlib

import numpy as np
import pytest

import _deemph_model as m
import _highcut_cases as hcc
import _highcut_model as hm
import _walk_cases as wc
import _walk_events as we

pytestmark = pytest.mark.gpu

F32 = np.float32
DEEMPH_CASES = [(s, nseg) for s in wc.SHAPES for nseg in sorted({k for k, _ in wc.lengths(s[1])})]
DEEMPH_50 = [(s, nseg) for s in ((0, 4), (33, 31), (256, 1)) for nseg in (2, 65, 1025)]


def same_bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (a.shape, b.shape, msg)
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb, err_msg="NaN positions " + msg)
    np.testing.assert_array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb], err_msg=msg)


@pytest.fixture()
def shape_option(fmrx):
    """Sets the process-wide lane shape, and puts the built-in one back."""
    def set_shape(W, L, mode=0):
        fmrx.set_option("deemph_warmup", W)
        fmrx.set_option("deemph_segment", L)
        fmrx.set_option("deemph_mode", mode)
    yield set_shape
    set_shape(-1, -1, 0)


def case_id(c):
    return f"{wc.shape_id(c[0])}-nseg{c[1]}"


# ---- 1. the de-emphasis stage function ------------------------------------------------------------------------------------
def stage_function(fmrx, shape_option, shape, nseg, tau):
    W, L = shape
    p, b0 = fmrx.deemphasisCoeffs(wc.FS, tau)
    events = []
    for n in [n for s, n in wc.lengths(L) if s == nseg]:
        c = wc.deemph_case(W, L, n, p, b0)
        events += c["events"]
        all_rows = len(c["x"])
        for rows in sorted({1, min(3, all_rows), all_rows}):
            shape_option(W, L)
            y, st, missed = fmrx.deemphasis(c["x"][:rows], p, b0, state=c["state"][:rows], pitch=n + 5)
            tag = f"(W, L) = ({W}, {L}), tau {tau}, rows {rows}, n {n}"
            same_bits(y, c["y"][:rows], tag)
            same_bits(st, c["state_out"][:rows], "state " + tag)
            print(f"{tag}: missed {missed}, model {int(c['missed'][:rows].sum())}")
            assert missed == int(c["missed"][:rows].sum()), tag
        shape_option(W, L, 1)                          # the serial kernel
        y, st, missed = fmrx.deemphasis(c["x"], p, b0, state=c["state"], pitch=n + 5)
        same_bits(y, c["y"], "serial kernel " + tag)
        same_bits(st, c["state_out"], "serial kernel, state " + tag)
        assert missed == 0
    print(f"events of the first rows: {we.table(we.total(events))}")


@pytest.mark.parametrize("case", DEEMPH_CASES, ids=case_id)
def test_deemph_stage_function(fmrx, shape_option, case):
    """rows 1, 3 and all of the case's (70 where rows change inside a workgroup of the segments kernel), a pitch larger than n,
    a carried state: output, state and miss count are the model's; the serial kernel gives the same bits and counts nothing."""
    stage_function(fmrx, shape_option, *case, 75.0)


@pytest.mark.parametrize("case", DEEMPH_50, ids=case_id)
def test_deemph_stage_function_at_50_us(fmrx, shape_option, case):
    stage_function(fmrx, shape_option, *case, 50.0)


@pytest.mark.parametrize("shape", [(40, 16), (33, 31), (0, 4), (256, 1)], ids=wc.shape_id)
def test_deemph_stream_in_unequal_calls(fmrx, shape_option, shape):
    """A stream cut into calls of 1, L - 1, W + L + 1, 3 samples and the rest, the state carried by the caller, equals one call
    and the model's serial walk.  With W > L the carried state is loaded by ceil(W / L) + 1 lanes of a row: row 1 carries a
    NaN, which every output of that row must then be."""
    W, L = shape
    shape_option(W, L)
    p, b0 = fmrx.deemphasisCoeffs(wc.FS, 75.0)
    cuts = [k for k in (1, L - 1, W + L + 1, 3) if k > 0]
    n = sum(cuts) + 5 * L + 2 * W + 7
    x, state, kinds = wc.inputs(W, L, n, 7)
    state[1] = [0.125, np.nan]
    whole, wstate, wmissed = fmrx.deemphasis(x, p, b0, state=state)
    want, sstate = m.serial(x, p, b0, state)
    same_bits(whole, want)
    same_bits(wstate, sstate)
    assert np.isnan(whole[1]).all() and np.isnan(wstate[1, 1])
    st, mst, at, out, misses = state, state, 0, [], []
    for k in cuts + [n - sum(cuts)]:
        y, st, ms = fmrx.deemphasis(x[:, at:at + k], p, b0, state=st)
        wy, mst, wms, _ = m.parallel(x[:, at:at + k], p, b0, mst, W, L)
        same_bits(y, wy, f"call of {k} at {at}")
        same_bits(st, mst, f"state behind the call of {k} at {at}")
        assert ms == wms, (k, at)
        misses.append(ms)
        out.append(y)
        at += k
    same_bits(np.concatenate(out, axis=1), whole)
    same_bits(st, wstate)
    print(f"{wc.shape_id(shape)}: calls of {cuts} and the rest of {n} samples miss {misses}, one call {wmissed}")


# ---- 2. de-emphasis through the pipeline, one large call -------------------------------------------------------------------
def _rows_of(out, channels):
    return np.stack([out["audio_l"], out["audio_r"]]) if channels == 2 else out["audio"][None, :]


SILENT = {"last 5 blocks": (12, 17), "first 16 blocks": (0, 16), "last block": (16, 17)}


@pytest.mark.parametrize("silent", list(SILENT))
@pytest.mark.parametrize("W,L", [(8, 2), (256, 1)])
@pytest.mark.parametrize("channels", [1, 2])
def test_pipeline_one_large_call(fmrx, channels, W, L, silent):
    """One call of 17 reference blocks through a handle with de-emphasis on and one with it off, wrapping and saturating: more
    than 8193 segments per row.  f32, PCM, the carried state and the diagnostics are the model's on the off handle's rows.
    Digital silence (byte 128; the audio dies away to +0: the silence onset) in the last 5 blocks; in the first 16, so that at
    (8, 2) the first window is clean and every miss is found, and f32 and PCM rewritten, in the second one; in the last block
    only, so that the repairs chain from the first window into the second."""
    nblk, tau = 17, 75.0
    bb = fmrx.modeParams(0).block_bytes

    def make(on):
        pl = fmrx.Pipeline(0, channels, max_block_bytes=nblk * bb)
        pl.set_option("deemph_warmup", W)
        pl.set_option("deemph_segment", L)
        if on:
            pl.set_deemphasis(tau)
        return pl

    iq = importlib.import_module(fmrx.__name__ + ".synth").synth_fm_u8(nblk * bb // 2, rf_Fs=float(fmrx.modeParams(0).rf_Fs))
    iq[SILENT[silent][0] * bb:SILENT[silent][1] * bb] = 128
    model = None
    for wrap in (True, False):
        on, off = make(True), make(False)
        p, b0 = fmrx.deemphasisCoeffs(on.params.audio_Fs, tau)
        o_on, o_off = on.process(iq, wrap=wrap), off.process(iq, wrap=wrap)
        x = _rows_of(o_off, channels)
        n = x.shape[1]
        assert (n + L - 1) // L > 8193
        if model is None:
            spec = m.speculate(x, p, b0, None, W, L)
            model = (x, spec) + m.parallel_rows(x, p, b0, None, W, L, spec=spec)
        same_bits(x, model[0], "the off handle's rows, wrapping and saturating")
        spec, want, st, missed, segs = model[1:]
        tag = f"{channels} channels, (W, L) = ({W}, {L}), silent: {silent}, wrap {wrap}"
        same_bits(_rows_of(o_on, channels), want, tag)
        pcm = np.stack([fmrx.pcm16(r, wrap=wrap) for r in want], axis=1).reshape(-1)
        np.testing.assert_array_equal(o_on["pcm16"], pcm, err_msg="pcm " + tag)
        assert on.deemph_diagnostics() == (segs, int(missed.sum())), tag
        same_bits(on.get_state()[-2 * channels:], st.reshape(-1), "carried state " + tag)
    _, _, events, found = wc.device_order(x, np.zeros((channels, 2), F32), spec, p, b0, L)
    total = we.total(events)
    print(f"{channels} channel(s), (W, L) = ({W}, {L}), silent: {silent}, {n} samples: {we.table(total)}")
    changed = [np.flatnonzero(~m.same(spec[0][r], want[r])) for r in range(channels)]
    if (W, L) == (8, 2) and silent == "first 16 blocks":
        assert total["miss_in_later_window"] >= channels and all(f[0][2] > 8193 for f in found)
        assert all(len(c) and c.min() >= 8193 * L for c in changed)      # samples rewritten, all of them behind the first window
    if (W, L) == (8, 2) and silent == "last block":
        assert total["chain_over_window"] >= channels and all(len(c) and c.max() >= 8193 * L for c in changed)


# ---- 3. the high-cut ---------------------------------------------------------------------------------------------------------
HIGHCUT_CASES = wc.highcut_cases()
FORCED = {wc.highcut_id(c) for c in (HIGHCUT_CASES[4], HIGHCUT_CASES[13])}   # cases that go in and out of the serial kernel


@pytest.mark.parametrize("case", HIGHCUT_CASES, ids=wc.highcut_id)
def test_highcut_six_calls(fmrx, oracle, case):
    """Six calls whose records move the pole inside a call, bring it down to 0 and up to p_max, the filter state carried: status,
    output, PCM and diagnostics are hm's at the case's lane shape.  Two of the cases run calls 1, 2 and 4 through the serial
    kernel (fmrx_highcut_set_force): the same bits, nothing counted."""
    c = case
    _, ctl, hc = hcc.make(fmrx, c["N"], c["ac"], c["n"], "fast", (c["W"], c["L"]))
    recs = hcc.records(ctl, c["N"])
    model = wc.HighcutWalk(ctl, c["N"], c["ac"], (c["W"], c["L"]))
    events = []
    for k in range(hcc.CALLS):
        audio, _ = wc.highcut_inputs(c, k)
        forced = wc.highcut_id(c) in FORCED and k in (1, 2, 4)
        hc.force_serial(forced)
        out = hc.process(recs[k], audio, want_f32=c["f32"], want_pcm=c["pcm"], wrap=c["wrap"], in_place=c["in_place"])
        want = model.call(recs[k], audio, counted=not forced)
        hcc.check_call(oracle, out, hc, model, want, c["wrap"], c["f32"], c["pcm"])
        events += model.last["events"]
    print(f"{wc.highcut_id(c)}: missed {model.missed} of {model.segments}; events of the first rows: {we.table(we.total(events))}")
    hc.close()
