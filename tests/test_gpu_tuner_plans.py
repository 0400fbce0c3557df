"""Every launch plan of the wideband tuner's matrix kernels on the device, bit for bit against the integer models
(tests/_tuner_model.py at U = 1, tests/_tuner_rational_model.py): the paths the other tuner tests do not reach.

  * a workgroup that walks more than one step (tuner_plan_info gives a workgroup ceil(n_steps * rows / 2048) steps): from the
    second step on every kernel re-stages its window behind a barrier, and the rational kernels flush and reuse their per-wave
    output buffer.  4099 steps on one row of workgroups, and 820 steps on five rows: three steps per workgroup, a ragged end.
  * every plan class of the rational kernels at its edge: the direct-store path (S16 with a large U and D), the largest LDS the
    plan accepts (163 776 bytes), the 8-bit formats' largest, and the shapes 16 or 32 bytes under the two-per-CU limit.
  * rates: every integer R from 2 to 32 (odd R, R < 4), U = 5, 7, 23, 24 at the ends and the middle of D, every count of stored
    K-steps per image for both kernel sets, 16 and 17 channels.

Every case first holds Tuner.plan() against the plan it was written for (tests/_tuner_plan_shapes.py, which
tests/test_tuner_plan_host.py holds against the product's host arithmetic on the CPU).  The generic kernels run the same
cases (tuner_variant); one model run serves both variants of a case.  The helpers are tests/test_gpu_tuner_rational.py's: at
U = 1, D <= 32 its pair() makes the integer tuner's handle and the rational model is the integer model."""
import numpy as np
import pytest

import _tuner_formats_model as fm
import _tuner_plan_shapes as ps
from test_gpu_tuner_rational import FMT_NAMES, channel_plan, pair, prototype, random_raw, same_call, set_both
from test_gpu_tuner_rational import variant  # noqa: F401  (the fixture: both kernel sets)

pytestmark = pytest.mark.gpu

FORMATS = [fm.U8, fm.S8, fm.S16]
fmt_id = lambda f: FMT_NAMES[f] if isinstance(f, int) and f in FMT_NAMES else None   # noqa: E731


class SharedModel:
    """One run of a case's model for both variants: the first pass computes and records every call's rows and levels, a later
    pass of the same calls replays them (the model is deterministic, and for the long calls it is most of a case's time)."""
    cases = {}

    @classmethod
    def of(cls, key, model):
        m = cls.cases.pop(key, None)
        if m is None:
            m = cls.cases[key] = cls(model)
        else:
            m.at = 0
        return m

    def __init__(self, model):
        self.model, self.log, self.at, self.U = model, [], None, model.U
        self.clipped, self.power = model.clipped, model.power

    def set_channel_ints(self, *a):
        if self.at is None:
            self.model.set_channel_ints(*a)

    def reset(self):
        if self.at is None:
            self.model.reset()

    def process(self, values):
        if self.at is None:
            out = self.model.process(values)
            self.log.append((out, self.model.clipped.copy(), self.model.power.copy()))
        else:
            self.at += 1
            assert self.at <= len(self.log), "the other variant's run of this case, which computed the model, did not finish"
        out, self.clipped, self.power = self.log[-1 if self.at is None else self.at - 1]
        return out


def make(fmrx, oracle, variant, row, max_wide, seed):
    """tuner, shared model, Fs_w, h, rng of a row of the shape table, the channels set to channel_plan's"""
    U, D, T, fmt, N = row["U"], row["D"], row["T"], row["fmt"], row["N"]
    Fs_w, h = prototype(oracle, U, D, T)
    tuner, model = pair(fmrx, U, D, h, N, max_wide, fmt)
    model = SharedModel.of((ps.row_id(row), max_wide, seed), model)
    rng = np.random.default_rng(seed)
    for c, (f_c, gain) in enumerate(channel_plan(N, Fs_w, rng)):
        set_both(fmrx, tuner, model, c, h, Fs_w, f_c, gain)
    return tuner, model, Fs_w, h, rng


def hold_plan(tuner, variant, row, n_wide):
    """the call runs the kernel, the output path and the LDS the case was written for"""
    p = tuner.plan(n_wide)
    if variant == "generic":
        assert not p["matrix"] and p["tiles"] == 0 and (p["grid_x"], p["grid_y"]) == (row["N"], (n_wide // row["D"] * row["U"] + 255) // 256), p
        return p
    if row.get("any_plan"):
        assert p["matrix"] and p["tiles"] >= 1, p
        return p
    assert p["matrix"] and (p["tiles"], p["via_lds"]) == (row["tiles"], row["via_lds"]), p
    assert (2 if p["lds_bytes"] <= ps.TWO_PER_CU else 1) == row["per_cu"] and p["lds_bytes"] <= ps.ONE_PER_CU, p
    if row["lds_bytes"] is not None:
        assert p["lds_bytes"] == row["lds_bytes"], p
    if row["n_steps"] is not None and n_wide == row["n_wide"]:
        assert (p["n_steps"], p["steps_per_wg"], (p["grid_x"], p["grid_y"])) == (row["n_steps"], row["steps_per_wg"], row["grid"]), p
    return p


def stream_of_calls(fmrx, oracle, variant, row, periods, seed):
    """tests/test_gpu_tuner_rational.py's test_device_bytes_equal_the_model on a row: calls of D x periods wide samples, then
    set_channel, then reset"""
    D, N, fmt = row["D"], row["N"], row["fmt"]
    tuner, model, Fs_w, h, rng = make(fmrx, oracle, variant, row, max(periods) * D, seed)
    for k in periods:
        hold_plan(tuner, variant, row, k * D)
    values = random_raw(rng, 2 * D * sum(periods), fmt)
    pos = 0
    for k in periods:
        same_call(tuner, model, values[pos:pos + 2 * D * k], f"call of {k} periods")
        pos += 2 * D * k
    set_both(fmrx, tuner, model, N - 1, h, Fs_w, -0.2 * Fs_w, 2.0)
    set_both(fmrx, tuner, model, 0, h, Fs_w, 0.31 * Fs_w, 0.9)
    same_call(tuner, model, values[:2 * D * min(17, max(periods))], "after set_channel")
    tuner.reset()
    model.reset()
    same_call(tuner, model, values[2 * D * 3:2 * D * (3 + periods[-2])], "after reset")
    tuner.close()


# ---- C1: several steps per workgroup -------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ps.MULTI_STEP + [ps.MULTI_STEP_ROWS], ids=ps.row_id)
def test_a_workgroup_walks_three_steps(fmrx, oracle, variant, row):
    """One call of 4099 steps less a few outputs on 3 channels (820 steps on 70 channels: five rows of workgroups): every
    workgroup but the last walks three steps, the last step of the call is ragged.  A short call in front leaves a history and
    a counter.  Whole rows and both level counters against the model.  Model time on the CPU: 0.5 .. 2.3 s per case, the five-row case 1.5 s (29 M output bytes),
    once for both variants."""
    D, fmt, n_wide = row["D"], row["fmt"], row["n_wide"]
    tuner, model, Fs_w, h, rng = make(fmrx, oracle, variant, row, n_wide, 1)
    p = hold_plan(tuner, variant, row, n_wide)
    if variant == "mfma":
        assert p["steps_per_wg"] >= 3 and p["n_steps"] % p["steps_per_wg"] != 0
        assert (n_wide // D * row["U"]) % (128 * row["U"] * row["tiles"]) != 0, "the last step is not ragged"
    same_call(tuner, model, random_raw(rng, 2 * D * 3, fmt), "three periods in front")
    same_call(tuner, model, random_raw(rng, 2 * n_wide, fmt), "the long call")
    assert model.clipped[2] > 0, "the clipping gain did not clip"
    tuner.close()


# ---- C2: every plan class and its edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ps.PLAN_CLASSES, ids=ps.row_id)
def test_every_plan_class_at_its_edge(fmrx, oracle, variant, row):
    stream_of_calls(fmrx, oracle, variant, row, ps.class_periods(row), 2)


def test_direct_stores_with_one_channel_in_the_second_row_of_workgroups(fmrx, oracle, variant):
    stream_of_calls(fmrx, oracle, variant, ps.DIRECT_17_CHANNELS, (1, 3, 40, 300), 3)


def test_direct_stores_into_a_pitch_larger_than_the_row(fmrx, oracle, variant):
    """direct stores are the path that could write past a ragged row end: 131 periods (two steps; the row is 5240 bytes, 8 past
    a 16-byte piece) into rows 5280 bytes apart, the gaps pre-filled; what lies between the rows is not written"""
    import torch
    row = ps.DIRECT_PITCH
    U, D, N, fmt, periods, pitch = row["U"], row["D"], row["N"], row["fmt"], 131, 5280
    tuner, model, Fs_w, h, rng = make(fmrx, oracle, variant, row, D * periods, 4)
    p = hold_plan(tuner, variant, row, D * periods)
    assert variant == "generic" or p["n_steps"] == 2
    n_row = 2 * U * periods
    assert tuner.n_out_bytes(D * periods) == n_row and n_row % 16 == 8 and pitch % 16 == 0 and pitch > n_row + 16
    cap = random_raw(rng, 2 * D * periods, fmt)
    d_out = torch.full((N * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    d_wide = torch.from_numpy(cap.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    tuner.process_dev(d_wide.data_ptr(), D * periods, d_out.data_ptr(), pitch)
    want = model.process(cap)
    cl, pw = tuner.levels()
    torch.cuda.synchronize()
    assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power)
    got = d_out.cpu().numpy().reshape(N, pitch)
    assert np.array_equal(got[:, :n_row], want)
    assert np.all(got[:, n_row:] == 0xA5)
    tuner.close()


# ---- C3: rates -------------------------------------------------------------------------------------------------------
INTEGER_CALLS = (1, 7, 130, 515)     # outputs per channel and call; at U = 1 a period is one output


@pytest.mark.parametrize("fmt", FORMATS, ids=fmt_id)
@pytest.mark.parametrize("R", ps.INTEGER_RATES)
def test_every_integer_rate(fmrx, oracle, variant, R, fmt):
    """R = 2, 3 (tuner_mac's walk over the padded window at D < 4) and every odd R (one pad piece per D) among them; the
    shortest filter, one that reaches two samples past 2 R, and the longest"""
    for T in ps.integer_taps(R):
        stream_of_calls(fmrx, oracle, variant, ps.integer_row(R, T, fmt), INTEGER_CALLS, 5)


def stream_at(fmrx, oracle, variant, U, D, T, fmt, N, periods, seed):
    """a rate case: whatever plan the shape has (tests/test_tuner_plan_host.py holds that it is a matrix kernel's)"""
    stream_of_calls(fmrx, oracle, variant, dict(ps.plan_row(U, D, T, fmt, None, None, None, N=N), any_plan=True), periods, seed)


@pytest.mark.parametrize("fmt", [fm.U8, fm.S16], ids=fmt_id)
@pytest.mark.parametrize("U,D", ps.rational_rates())
def test_rational_rates_at_the_ends_of_the_range(fmrx, oracle, variant, U, D, fmt):
    for T in ps.rational_taps(U, D):
        stream_at(fmrx, oracle, variant, U, D, T, fmt, 5, (1, 3, 40, 300), 6)


@pytest.mark.parametrize("fmt", [fm.U8, fm.S16], ids=fmt_id)
@pytest.mark.parametrize("ksp", range(1, 10))
def test_every_count_of_stored_k_steps(fmrx, oracle, variant, ksp, fmt):
    for U, D, T in (ps.KSP_INTEGER[ksp], ps.KSP_RATIONAL[ksp]):
        stream_at(fmrx, oracle, variant, U, D, T, fmt, 5, (1, 7, 130, 600), 7)


@pytest.mark.parametrize("N", [16, 17])
@pytest.mark.parametrize("U,D,T", ps.SIXTEEN_SEVENTEEN)
def test_sixteen_and_seventeen_channels(fmrx, oracle, variant, U, D, T, N):
    for fmt in FORMATS:
        stream_at(fmrx, oracle, variant, U, D, T, fmt, N, (1, 7, 130, 300), 8)


def test_plan_argument_checks(fmrx, oracle):
    """fmrx_tuner_plan: a null handle, a null result and every n_wide process_dev would refuse are FMRX_EINVAL; the plan is the
    same before and after a call, and under tuner_variant = generic it says so"""
    Fs_w, h = prototype(oracle, 6, 25, 200)
    t = fmrx.Tuner.rational(6, 25, h, 2, 2500)
    for n_wide in (0, 30, 2525, 5000):
        with pytest.raises(fmrx.FmrxError, match="n_wide") as e:
            t.plan(n_wide)
        assert e.value.code == fmrx.EINVAL
    info = fmrx.TunerPlanInfo()
    assert fmrx.lib.fmrx_tuner_plan(None, 2500, fmrx.C.byref(info)) == fmrx.EINVAL
    assert fmrx.lib.fmrx_tuner_plan(t._h, 2500, None) == fmrx.EINVAL
    before = t.plan(2500)
    assert before == dict(matrix=True, tiles=1, via_lds=True, lds_bytes=before["lds_bytes"], n_steps=1, steps_per_wg=1, grid_x=1, grid_y=1)
    assert before["lds_bytes"] <= ps.TWO_PER_CU
    t.process(np.full(2 * 2500, 128, np.uint8))
    assert t.plan(2500) == before
    fmrx.set_option("tuner_variant", "generic")
    try:
        g = fmrx.Tuner.rational(6, 25, h, 2, 2500)
    finally:
        fmrx.set_option("tuner_variant", "mfma")
    assert g.plan(2500) == dict(matrix=False, tiles=0, via_lds=False, lds_bytes=0, n_steps=0, steps_per_wg=0, grid_x=2, grid_y=3)
    assert t.plan(2500) == before
