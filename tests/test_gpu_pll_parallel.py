"""The parallel-in-time PLL on the device (csrc/kernels_pll.hip: pll_lti_chunks_kernel, pll_segments_kernel,
pll_repair_kernel) checked segment by segment against tests/_pll_parallel_model.py, through the stage entry
fmrx.fmPllParallel, which runs what a warm pipeline's PLL stage runs and returns the segment records: per segment its end
state, the (integ, phase) its outputs were computed from (the basis) and how often the repair walked it.

Per call, from the records (check_call):
  own lane     a segment the repair never walked ends BIT FOR BIT where walk() ends from its recorded basis, its trigOffset
               is exact, and its NCO row is within pm.NCO_EPS of cos(2 pi r_model).  Segments whose walk holds an undetermined
               step (tests/_pll_model.py) are exempt: at most 1 % of a call's segments, none in inputs without zeros.
  seams        every basis that is not bit-equal to its predecessor's FINAL end is within the call's own tolerances of it (the
               model's tolerances, which the entry's equal bit for bit); the final mask is all zero; no such difference
               exceeds the reported maxima.
  replay       lanes that start at the block's start chain bit for bit (basis == predecessor's end) and, being the serial
               recurrence itself, equal walk() bit for bit from the predecessor's end; so does segment 0 from the reset state.
               From a carried state segment 0 starts on fr = atan2f(fbQ, fbI) / 2 pi of the device, which the model cannot
               restate: it is held to the merge tolerance of walk(), like every
  re-walked    segment: the repair rebuilds fr from the hardware cos / sin pair with atan2f, so the end is within the merge
               tolerance -- the project's definition of "the same trajectory" -- of walk() from the recorded basis, and that
               basis is its predecessor's FINAL end bit for bit: a repaired stretch is one serial walk.
  state        the returned state is the last record; the repaired count is the sum of the records' walk counts.
Linear start (pll_warmup 0: the basis IS lti_start): within one float32 ulp + 1e-9 of the model, which restates the kernel's
float64 operations in the kernel's order.  Measured on an MI355X: largest difference 0 -- every such basis of the three
fixtures (536 segments) equals the model's bit for bit.  Largest NCO difference of this file: 1.25e-7 (pm.NCO_EPS is 5e-7).

Under the rule pll_repair_kernel had before (a walked segment re-judged by its lane's warm-up start, to the tolerances) a
segment could come to rest on a predecessor's end that a later round replaced.  On an MI355X, with that rule put back, the
drop-out fixture (64 walks, 18 segments walked twice, from either start state) and 60 random streams with drop-outs of 3
to 400 samples, noise up to 0.4 and phase jumps showed no such segment: every walked segment's end was where the model's
walk from its predecessor's FINAL end ends (phase equal, integrator within 1e-9).  The case was not reproduced on the
device; the rule is closed by construction: a walked segment's basis is its predecessor's final end bit for bit."""
import math

import numpy as np
import pytest

import _pll_model as pm
import _pll_parallel_model as pp

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
C = pm.coef(19e3, 240e3)
N_FIRST = 4096
MEASURED = {"nco": 0.0, "lti": 0.0}


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@pytest.fixture
def options(fmrx):
    """Set process-wide PLL options for one test; the built-in values afterwards."""
    names = ("pll_start", "pll_warmup", "pll_segment")
    before = {k: fmrx.get_option(k) for k in names}

    def set_(**kw):
        for k in names:
            fmrx.set_option(k, kw.get(k, before[k]))
    yield set_
    for k, val in before.items():
        fmrx.set_option(k, val)


def entry(fmrx, v, state, off_hint):
    return fmrx.fmPllParallel(v, state, 19e3, 240e3, 2.0, 0.0, 0.01, off_hint)


@pytest.fixture(scope="module")
def carried(fmrx):
    """The state a first call of 4096 samples of the clean tone left (default lane shape), from the reset state."""
    _, st, info, _ = entry(fmrx, pp.tone(N_FIRST, seed=1), pp.RESET, 0.0)
    assert info["nseg"] == N_FIRST // 64 and st[5] == N_FIRST
    return st


@pytest.fixture(scope="module")
def inputs():
    return {0: pp.fixtures(0), N_FIRST: pp.fixtures(N_FIRST)}


def expected_shape(start, warmup, segment, off_hint, n):
    """L, W, lti as k_fm_pll_parallel derives them from the options."""
    L, W = 64, 512
    if 0 <= warmup <= 65536:
        W = warmup // 4 * 4
    if 32 <= segment <= 65536:
        L = segment // 4 * 4
    lti = start == 1 and off_hint >= 0 and C.w * (off_hint + n) < 4194304.0
    if lti:
        if warmup < 0:
            W = 64
        W, L = (W + 63) // 64 * 64, 64
    return L, W, lti


def check_call(fmrx, v, state, off_hint, shape, has_zeros=False, tag=""):
    """One call through the entry, every assertion of the module docstring; returns (nco, state, info, records, facts)."""
    v, state = np.asarray(v, F32), np.asarray(state, F32)
    n = len(v)
    nco, st, info, rec = entry(fmrx, v, state, off_hint)
    L, W, lti = shape
    assert (info["L"], info["W"], info["lti"]) == (L, W, lti), (tag, info)
    assert nco[0] == state[4]
    if n < 4 * L:                                           # the serial fast kernel
        assert info["nseg"] == 0 and len(rec["end"]) == 0
        return nco, st, info, rec, {}
    nseg = (n + L - 1) // L
    end, basis, walks = rec["end"], rec["basis"], rec["walks"]
    assert info["nseg"] == nseg and end.shape == (nseg, 6)
    tol = pp.tolerances(state, n, C, lti)
    assert bits(info["tol_phase"]) == bits(tol[0]) and bits(info["tol_integ"]) == bits(tol[1]), (tag, info, tol)
    assert not info["mask"].any(), f"{tag}: segments left flagged {np.flatnonzero(info['mask'])}"
    a = np.arange(nseg) * L
    np.testing.assert_array_equal(end[:, 5], (state[5] + np.minimum(a + L, n).astype(F32)).astype(F32), err_msg=f"{tag}: trigOffset")
    np.testing.assert_array_equal(bits(st), bits(end[-1]), err_msg=f"{tag}: returned state vs last record")
    assert info["repaired"] == walks.sum() and (walks >= 0).all(), (tag, info["repaired"], walks.sum())

    pred = np.concatenate([state[None, :2], end[:-1, :2]])                  # what each segment's predecessor ended on
    chained = (bits(basis) == bits(pred)).all(axis=1)
    replay = a <= W
    assert chained[replay].all() and (walks[replay] == 0).all(), f"{tag}: lanes from the block's start do not chain bit for bit"
    # seams
    loose = np.flatnonzero(~chained)
    dp = pp.phase_dist(basis[loose, 1], pred[loose, 1])
    di = np.abs((basis[loose, 0] - pred[loose, 0]).astype(F32))
    bad = loose[~((dp <= tol[0]) & (di <= tol[1]))]
    assert len(bad) == 0, f"{tag}: {len(bad)} segments rest on a basis outside the tolerances of their predecessor's final end: {bad[:8]}"
    if len(loose):
        assert dp.max() <= info["max_dphase"] and di.max() <= info["max_dinteg"], (tag, dp.max(), di.max(), info)
    # every segment walked by the model from its recorded basis
    trig, m_integ, m_phase, und = pp.walk_all(basis[:, 0], basis[:, 1], state[5], v, L, C)
    exempt = und >= 0
    assert exempt.mean() <= pp.EXEMPT_CAP and (has_zeros or not exempt.any()), (tag, exempt.sum())
    reset_start = np.array_equal(bits(state), bits(pp.RESET))
    exact = (walks == 0) & ~exempt
    if not reset_start:
        exact[0] = False
    wrong = np.flatnonzero(exact & ((bits(end[:, 0]) != bits(m_integ)) | (bits(end[:, 1]) != bits(m_phase))))
    assert len(wrong) == 0, f"{tag}: {len(wrong)} of {exact.sum()} segments do not end where the model's walk from their basis ends: {wrong[:8]}"
    r = pm.nco_arg(trig, C).astype(F64)
    d = np.abs(nco[1:].astype(F64) - np.cos(2 * math.pi * r))
    rows = np.repeat(exact, L)[:n]
    worst = float(d[rows].max(initial=0.0))
    MEASURED["nco"] = max(MEASURED["nco"], worst)
    assert worst <= pm.NCO_EPS, f"{tag}: NCO off by {worst:.3e} in segment {int(np.argmax(np.where(rows, d, 0))) // L}"
    # re-walked segments (and segment 0 from a carried state): the same trajectory to the merge tolerance
    near = np.flatnonzero(~exact & ~exempt)
    off = ~pp.merged(end[near, 0], end[near, 1], m_integ[near], m_phase[near], tol)
    assert not off.any(), f"{tag}: re-walked segments {near[off][:8]} end outside the merge tolerance of the model's walk"
    assert (walks[near[near > 0]] > 0).all()
    assert chained[walks > 0].all(), f"{tag}: walked segments {np.flatnonzero(~chained & (walks > 0))[:8]} do not start on their predecessor's final end"
    facts = {"own": int(exact.sum()), "rewalked": int((walks > 0).sum()), "twice": int((walks > 1).sum()), "nco": worst, "repaired": int(info["repaired"])}
    print(f"{tag}: n {n} L {L} W {W} lti {lti}: {facts}, accepted maxima ({info['max_dphase']:.2e}, {info['max_dinteg']:.2e}) of "
          f"({float(tol[0]):.2e}, {float(tol[1]):.2e}); NCO max so far {MEASURED['nco']:.3e}")
    return nco, st, info, rec, facts


@pytest.mark.parametrize("start", ["reset", "carried"])
@pytest.mark.parametrize("name", ["tone", "jump", "dropouts", "zeros", "no_pilot"])
def test_default_lanes_every_input(fmrx, options, carried, inputs, name, start):
    """pll_start 1, W = 64: every crafted input from the reset state and from the state a first call left."""
    options()
    state, s0 = (pp.RESET, 0) if start == "reset" else (carried, N_FIRST)
    v, has_zeros = inputs[s0][name]
    *_, info, rec, facts = check_call(fmrx, v, state, float(s0), (64, 64, True), has_zeros, f"{name}/{start}")
    if name == "tone" and start == "carried":
        assert info["repaired"] == 0
    if name == "no_pilot":
        assert facts["rewalked"] >= 0.9 * info["nseg"]


@pytest.mark.parametrize("start", ["reset", "carried"])
def test_dropouts_are_repaired_more_than_once(fmrx, options, carried, inputs, start):
    """The drop-out fixture walks segments twice on the device as it does in the model -- the path on which a segment could
    come to rest on a predecessor's end that a later round replaced.  check_call's seam assertion (every basis against its
    predecessor's FINAL end, every walked segment chained to it bit for bit) is what fails there; see the module docstring
    for what the device showed under the earlier rule."""
    options()
    state, s0 = (pp.RESET, 0) if start == "reset" else (carried, N_FIRST)
    *_, facts = check_call(fmrx, inputs[s0]["dropouts"][0], state, float(s0), (64, 64, True), False, f"dropouts/{start}")
    assert facts["twice"] >= 1 and facts["repaired"] > facts["rewalked"]


@pytest.mark.parametrize("n", [255, 256, 257, 258, 259, 256 + 61, 64 * 80])
@pytest.mark.parametrize("start", ["reset", "carried"])
def test_shapes_short_and_ragged(fmrx, options, carried, n, start):
    """255: the serial fall-back (from the reset state: integ, phase, trigOffset equal the model's bit for bit, the NCO within
    NCO_EPS); 256 .. 317: the ragged last segment; 64 * 80: two waves, one seam judged by the repair kernel.  Clean tone and
    the same with a 40-sample drop-out (in the third segment; for two waves across their seam)."""
    options()
    state, s0 = (pp.RESET, 0) if start == "reset" else (carried, N_FIRST)
    clean = pp.tone(n, seed=5, start=s0)
    lo = 64 * 64 - 30 if n > 1000 else 150                   # across the seam between the two waves
    for kind, v in (("clean", clean), ("dropout", pp.with_dropouts(clean, [(lo, 40)], seed=5))):
        nco, st, info, _, _ = check_call(fmrx, v, state, float(s0), (64, 64, True), False, f"n {n}/{kind}/{start}")
        if n < 256 and start == "reset":
            trig, ms, und = pm.run(v, C)
            assert und == -1
            np.testing.assert_array_equal(bits(st[[0, 1, 5]]), bits([ms.integ[0], ms.phase[0], ms.off[0]]))
            assert np.abs(nco[1:] - pm.nco(trig, C)).max() <= pm.NCO_EPS


def test_past_the_strided_judge_loop(fmrx, options, carried):
    """n = 64 (64 * 256 + 70) + 3: 16455 segments, 258 waves -- more seams between waves than pll_repair_kernel has threads, a
    ragged end of 3; a drop-out sits on the seam the strided loop judges (segment 64 * 257) and one in the first wave."""
    options()
    n = 64 * (64 * 256 + 70) + 3
    v = pp.with_dropouts(pp.tone(n, seed=6, start=N_FIRST), [(2000, 40), (64 * 64 * 257 - 30, 40), (n - 700, 400)], seed=6)
    *_, info, rec, facts = check_call(fmrx, v, carried, float(N_FIRST), (64, 64, True), False, "long")
    assert rec["walks"][64 * 257] >= 1 and facts["rewalked"] >= 3


@pytest.mark.parametrize("start,warmup,segment", [(1, 0, -1), (1, 128, -1), (0, 512, 64), (0, 256, 128), (0, 64, 32)])
@pytest.mark.parametrize("name", ["tone", "dropouts", "zeros"])
def test_lane_shapes(fmrx, options, carried, inputs, name, start, warmup, segment):
    """pll_start 1 with W = 0 and 128; pll_start 0 (no drift record: the entry starts from a zeroed work area) with
    (W, L) = (512, 64), (256, 128), (64, 32).  At W = 0 every basis the repair did not replace IS the linear start: within
    one float32 ulp + 1e-9 of lti_start()."""
    options(pll_start=start, pll_warmup=warmup, pll_segment=segment)
    v, has_zeros = inputs[N_FIRST][name]
    shape = expected_shape(start, warmup, segment, N_FIRST, len(v))
    *_, info, rec, facts = check_call(fmrx, v, carried, float(N_FIRST), shape, has_zeros, f"{name}/start {start} W {warmup} L {segment}")
    if start == 1 and warmup == 0:
        s = np.flatnonzero(rec["walks"] == 0)[1:]
        assert len(s) > 0
        m_integ, m_phase = pp.lti_start(carried, pp.lti_records(v > 0, C, len(v)), s)
        for got, want, what in ((rec["basis"][s, 0], m_integ, "integ"), (rec["basis"][s, 1], m_phase, "phase")):
            d = np.abs(got.astype(F64) - want.astype(F64))
            MEASURED["lti"] = max(MEASURED["lti"], float(d.max()))
            print(f"linear start, {name}, {what}: {len(s)} segments, max |device - model| {d.max():.3e} (largest so far {MEASURED['lti']:.3e})")
            over = d > np.spacing(np.abs(want)).astype(F64) + 1e-9
            assert not over.any(), (what, s[over][:8], d[over][:8])


def test_first_start_form_past_the_hand_over(fmrx, options):
    """off_hint past 2^22 rad of trigArg under pll_start 1: the lanes start the first way (W = 512, no linear system).  The
    state is the reset state moved to trigOffset 8.5e6; ulp(trigArg) is 0.5 rad there."""
    options()
    off = 8.5e6
    state = pp.RESET.copy()
    state[5] = off
    v = pp.tone(64 * 80, seed=8, start=int(off))
    assert C.w * off > 4194304.0
    *_, info, _, _ = check_call(fmrx, v, state, off, (64, 512, False), False, "past 2^22 rad")
    assert not info["lti"]


def test_the_pipeline_runs_this_stage(fmrx, oracle, options):
    """A stereo pipeline, mode 0, plain calls: its second call's carrier_filt tap and the PLL state after its first call,
    through the stage entry with off_hint = the first call's n_if, give the second call's pll tap and PLL state bit for bit."""
    options()
    p = fmrx.modeParams(0)
    iq = oracle.synth_fm_u8(p.block_bytes, seed=0x3D74)
    pl = fmrx.Pipeline(0, 2)
    pl.process(iq[:p.block_bytes], want_pcm=False)
    state1, n_if = pl.get_state()[-6:].copy(), len(pl.read_tap("carrier_filt"))
    pl.process(iq[p.block_bytes:], want_pcm=False)
    car, want, state2 = pl.read_tap("carrier_filt"), pl.read_tap("pll"), pl.get_state()[-6:]
    nco, st, info, _ = entry(fmrx, car, state1, float(n_if))
    assert info["lti"] and info["nseg"] == len(car) // 64
    np.testing.assert_array_equal(bits(nco), bits(want))
    np.testing.assert_array_equal(bits(st), bits(state2))
