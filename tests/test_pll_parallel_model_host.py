"""The model of the parallel-in-time PLL (tests/_pll_parallel_model.py) checked on the CPU: its linear start against the
linear system stepped sample by sample, a lane's walk against the serial model, and that the bounds
tests/test_gpu_pll_parallel.py holds the device to can tell a subtly wrong kernel from a right one."""
import numpy as np
import pytest

import _pll_model as pm
import _pll_parallel_model as pp

F32, F64 = np.float32, np.float64
C = pm.coef(19e3, 240e3)


def locked_state(n_head=4096):
    """(state[6], fr) after a serial first stretch of the clean tone."""
    _, st, _ = pm.run(pp.tone(n_head, seed=1), C)
    return np.array([st.integ[0], st.phase[0], 1, 0, 1, st.off[0]], F32), st.fr[0]


def stepped_linear_system(v, state):
    """(integ, phase) in front of every 64th sample: the recurrence of kernels_pll.hip's comment, one sample at a time."""
    m = pp.lti_of(C)
    pos = v > 0
    phi, iota, off0 = float(state[1]) * pm.INV_2PI, float(state[0]) * pm.INV_2PI, float(state[5])
    th0 = float(F32(C.w * off0 + float(state[1]))) * pm.INV_2PI
    T = np.rint(th0) if pos[0] else np.rint(th0 - 0.5) + 0.5
    out = []
    for k in range(len(v)):
        if k % pp.CHUNK == 0:
            out.append((iota * pp.TWO_PI, phi * pp.TWO_PI))
        phi, iota = pp.lti_step(m, phi, iota, T - m.f * (off0 + k))
        if k + 1 < len(v) and pos[k + 1] != pos[k]:
            T += 0.5
    return np.array(out)


def bound_of_start(x):
    """What the GPU test allows between the device's linear start and the model's: one float32 ulp + 1e-9."""
    return np.spacing(np.abs(np.asarray(x, F32))).astype(F64) + 1e-9


@pytest.mark.parametrize("start", ["reset", "locked"])
def test_linear_start_is_the_stepped_system(start):
    """The 20-term start (with the block's true state near its start, and i == 0) equals the linear system stepped sample by
    sample from the block's start to 1e-6 rad, over 150 chunks (three workgroups of the chunk kernel) of a tone with a phase
    jump.  The bound is for a phase estimate of a few radians: its float32 rounding (2.4e-7 at 2 rad) is part of the
    difference, and so is what the 20 terms drop, (A^64)^20 = 5e-8 of the linear state's distance from the block's start.
    (A stretch of noise makes the staircase climb by whole turns the true loop never makes: the linear phase then stands
    tens of radians off, where one float32 step alone is 4e-6.)"""
    n = 64 * 150 + 37
    state = pp.RESET if start == "reset" else locked_state()[0]
    v = pp.with_dropouts(pp.tone(n, seed=4, start=int(state[5]), jump_at=5000, jump=2.0), [], seed=4)
    rec = pp.lti_records(v > 0, C, n)
    i = np.arange(n // 64 + 1)
    integ, phase = pp.lti_start(state, rec, i)
    want = stepped_linear_system(v, state)
    d = np.abs(np.stack([integ, phase], axis=1).astype(F64) - want)
    print(f"linear start vs stepping ({start}): max |d integ| {d[:, 0].max():.2e}, |d phase| {d[:, 1].max():.2e} rad")
    # float32 rounding of the result is part of the difference: phases of a few rad carry 2.4e-7
    assert d.max() <= 1e-6
    assert integ[0] == state[0] and phase[0] == state[1]


def test_warmed_up_lane_lands_on_the_serial_trajectory():
    """With W large (1024) a lane started from the linear system walks onto the serial model's trajectory: at its segment
    start it is within the merge tolerance of pm.run's state there, for every segment of the clean tone."""
    state, fr = locked_state()
    v = pp.fixtures(start=4096)["tone"][0]
    r = pp.simulate(v, state, C, W=1024, fr0=fr)
    assert r["repaired"] == 0
    s = pm.State(state[:1].copy(), state[1:2].copy(), state[5:6].copy(), np.array([fr], F32))
    serial = []
    for lo in range(0, len(v), pp.CHUNK):
        serial.append((s.integ[0], s.phase[0]))
        _, s, _ = pm.run(v[lo:lo + pp.CHUNK], C, s)
    serial = np.array(serial, F32)
    ok = pp.merged(r["basis"][:, 0], r["basis"][:, 1], serial[:, 0], serial[:, 1], r["tol"])
    assert ok.all(), np.flatnonzero(~ok)
    assert pp.phase_dist(r["end"][-1, 1], s.phase[0]) <= r["tol"][0]


def test_a_subtly_wrong_linear_start_leaves_the_bound():
    """A prefix shifted by one chunk, one dropped sign change, and a climb that ignores the next chunk's first sample each
    move the linear start of some chunk by more than the bound the GPU test holds it to (one float32 ulp + 1e-9)."""
    state, _ = locked_state()
    v = pp.fixtures(start=4096)["tone"][0]
    n = len(v)
    rec = pp.lti_records(v > 0, C, n)
    i = np.arange(1, n // 64)
    good = np.stack(pp.lti_start(state, rec, i), axis=1).astype(F64)
    bound = np.stack([bound_of_start(good[:, 0]), bound_of_start(good[:, 1])], axis=1)

    def moved(r):
        return (np.abs(np.stack(pp.lti_start(state, r, i), axis=1).astype(F64) - good) > bound).any()

    shifted = dict(rec, pre=np.roll(rec["pre"], 1))
    assert moved(shifted)
    dT = rec["dT"].copy()
    dT[90] -= 0.5                                            # one sign change not counted, in the second workgroup
    d = np.zeros(64 * len(rec["wgtot"]))
    d[:len(dT)] = dT
    d = d.reshape(-1, 64)
    dropped = dict(rec, dT=dT, pre=(np.cumsum(d, axis=1) - d).reshape(-1)[:len(dT)], wgtot=d.sum(axis=1))
    assert moved(dropped)
    blind = pp.lti_records(v > 0, C, n, look_ahead=False)
    assert (blind["dT"] != rec["dT"]).any() and moved(blind)


def test_one_ulp_of_ki_leaves_a_segments_end():
    """Ki one ulp off: some segment's end (integ, phase) after 64 steps is not the model's bit for bit -- what the GPU test
    asks of every lane's own walk."""
    state, _ = locked_state()
    v = pp.fixtures(start=4096)["tone"][0]
    rec = pp.lti_records(v > 0, C, len(v))
    integ, phase = pp.lti_start(state, rec, np.arange(len(v) // 64))
    base = pp.walk_all(integ, phase, state[5], v, 64, C)
    bumped = pm.Coef(C.Kp, np.nextafter(C.Ki, F32(1)), C.w, C.nco_scale, C.phase_adjust)
    other = pp.walk_all(integ, phase, state[5], v, 64, bumped)
    differ = (base[1].view(np.uint32) != other[1].view(np.uint32)) | (base[2].view(np.uint32) != other[2].view(np.uint32))
    print(f"Ki + 1 ulp: {differ.sum()} of {len(differ)} segment ends differ")
    assert differ.sum() > len(differ) // 2


def test_fixtures_exempt_share_and_double_repairs():
    """On the model alone: the fixtures without zeros hold no undetermined step, the one with a run of zeros keeps its
    segments with one under the cap, the drop-out fixture has segments walked twice by the repair, the clean tone none at
    all; both repair rules leave every basis within the tolerances of its predecessor's final end here (the rule before
    re-judged a re-walked segment by its lane's warm-up start)."""
    for start, state, fr in ((0, pp.RESET, 0.0), (4096,) + locked_state()):
        for name, (v, has_zeros) in pp.fixtures(start).items():
            r = pp.simulate(v, state, C, fr0=fr)
            share = (r["und"] >= 0).mean()
            print(f"start {start} {name}: repaired {r['repaired']}, walked twice {(r['walks'] > 1).sum()}, stale {len(r['stale'])}, "
                  f"undetermined share {share:.4f}")
            assert share <= pp.EXEMPT_CAP and (has_zeros or share == 0)
            assert len(r["stale"]) == 0
            if name == "dropouts":
                assert (r["walks"] > 1).sum() >= 10
            if name == "tone" and start:
                assert r["repaired"] == 0
            if name == "no_pilot":
                assert (r["walks"][1:] >= 1).mean() > 0.9


def test_tolerances_and_phase_distance():
    """pll_phase_tol / pll_integ_tol: base + 2 ulp and base + 6 (2) Ki ulp of the float32 trigArg at the block's end;
    pll_phase_dist forgets whole turns."""
    state = np.array([0, 0, 1, 0, 1, 5120], F32)
    tp, ti = pp.tolerances(state, 5120, C, True)
    u = 2.0 ** (np.floor(np.log2(C.w * 10240)) - 23)
    assert tp == F32(F32(1e-2) + F32(2 * u)) and abs(float(ti) - (1e-4 + 6 * float(C.Ki) * u)) < 1e-11
    assert pp.tolerances(state, 5120, C, False)[1] < ti
    assert pp.phase_dist(F32(6.3), F32(0.01)) < 0.01 and abs(float(pp.phase_dist(F32(1.0), F32(-1.0))) - 2.0) < 1e-6
