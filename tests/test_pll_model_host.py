"""The fast-PLL model (tests/_pll_model.py) checked on the CPU: its phase detector against the arctangent it replaces, its
zero / infinity path against libm's atan2f, and its loop against the reference's (the oracle's fm_pll).  The GPU side is
tests/test_gpu_pll_exact.py."""
import math

import numpy as np
import pytest

import _pll_model as pm

F32, F64 = np.float32, np.float64


def wrap_pi(d):
    """d turned into (-pi, pi]."""
    d = np.asarray(d, F64)
    r = d - 2 * math.pi * np.round(d / (2 * math.pi))
    return np.where(r <= -math.pi, r + 2 * math.pi, r)


def near(points, k=40):
    """float32 fr within a few hundred ulps either side of each point (clipped to [-0.5, 0.5])."""
    out = []
    for p in points:
        x = F32(p)
        up, dn = x, x
        for _ in range(k):
            up, dn = np.nextafter(up, F32(1)), np.nextafter(dn, F32(-1))
            out += [up, dn]
        out.append(x)
    fr = np.array(out, F32)
    return fr[np.abs(fr) <= 0.5]


def test_loop_constants():
    """Kp, Ki, w as make_coef (kernels_pll.hip) and fmPLL derive them: float products, freq/Fs a float division."""
    c = pm.coef(19e3, 240e3)
    assert c.Kp == F32(F32(0.01) * F32(2.666)) and c.Ki == F32(F32(F32(0.01) * F32(0.01)) * F32(3.555))
    assert c.w == 2 * 3.14159265358979323846 * float(F32(19e3) / F32(240e3))
    assert c.w != 2 * math.pi * 19e3 / 240e3                 # the float division shows in the double


def test_closed_form_detector_is_the_arctangent():
    """eD of an ordinary sample equals float64 atan2(-v sin 2 pi fr, v cos 2 pi fr), turned into (-pi, pi], to within 2 ulp
    of float32: random fr, both signs of v over the ordinary range, fr right at and around +-0.25 and +-0.5 (and 0)."""
    rng = np.random.default_rng(5)
    fr = np.concatenate([rng.uniform(-0.5, 0.5, 20000).astype(F32), near([0.25, -0.25, 0.5, -0.5, 0.0, 0.125, -0.375])])
    mag = np.exp(rng.uniform(math.log(2e-20), math.log(5e19), len(fr)))
    for sign in (1.0, -1.0):
        v = (sign * mag).astype(F32)
        assert pm.ordinary(v).all()
        eD = pm.closed_form_detector(v, fr).astype(F64)
        t = 2 * math.pi * fr.astype(F64)
        want = np.arctan2(-v.astype(F64) * np.sin(t), v.astype(F64) * np.cos(t))
        d = wrap_pi(eD - want)
        # (+ 1e-12: the float64 reference's own error, e.g. sin(2 pi * 0.5) = 1.2e-16, not 0)
        tol = 2 * np.spacing(np.abs(want).astype(F32)).astype(F64) + 1e-12
        bad = np.flatnonzero(np.abs(d) > tol)
        assert len(bad) == 0, (sign, fr[bad[:5]], eD[bad[:5]], want[bad[:5]])
        assert (np.abs(eD) <= F32(math.pi) * (1 + 2 ** -23)).all()


@pytest.mark.parametrize("v", [0.0, -0.0, np.inf, -np.inf])
def test_zero_and_inf_path_is_libm(oracle, v):
    """v = +-0, +-inf (the library path): eD is libm's atan2f of the signed zeros / infinities v*cos, v*(-1*sin) in every
    quadrant of fr -- against the oracle's call of the C library and against the IEEE values (+-0, +-pi, +-pi/4, +-3 pi/4);
    fr next to the quadrant edges is undetermined (0 only for an infinite v: a zero v there gives +0 or -0, both harmless)."""
    fr = np.array([0.1, 0.2, 0.3, 0.45, -0.1, -0.2, -0.3, -0.45, 0.2499, -0.2501, 0.4999, -0.4999, 0.01, -0.01], F32)
    vv = np.full(len(fr), v, F32)
    eD, und = pm.library_detector(vv, fr)
    assert not und.any()
    t = 2 * math.pi * fr.astype(F64)
    fbI, fbQ = np.cos(t).astype(F32), np.sin(t).astype(F32)
    eI, eQ = (vv * fbI).astype(F32), (vv * (F32(-1) * fbQ)).astype(F32)
    np.testing.assert_array_equal(eD.view(np.uint32), oracle.libm("atan2f", eQ, eI).view(np.uint32))
    np.testing.assert_array_equal(eD.view(np.uint32), np.arctan2(eQ.astype(F64), eI.astype(F64)).astype(F32).view(np.uint32))
    edge = np.array([0.25 + 2 ** -22, -0.25 - 2 ** -22, 0.5 - 2 ** -22, -0.5 + 2 ** -22, 2 ** -22], F32)
    _, und = pm.library_detector(np.full(len(edge), v, F32), edge)
    np.testing.assert_array_equal(und, [True] * 4 + [bool(np.isinf(v))])
    # NaN and non-ordinary finite samples: the hardware sine / cosine's magnitudes enter -- never determined
    _, und = pm.library_detector(np.array([np.nan, 1e-30, -3e-41, 2e20], F32), np.full(4, 0.1, F32))
    assert und.all()


def test_run_steps_and_carries_state():
    """run() in one piece equals run() over pieces with the state carried (the model's own seams are exact); a zero
    sample from the reset state (fr = 0) is determined; the final state holds off = samples walked."""
    rng = np.random.default_rng(9)
    c = pm.coef()
    v = np.where(rng.random((3, 3000)) < 0.5, F32(1), F32(-1)).astype(F32)
    v[1, :700] = 0.0                                         # silence, then a signal
    v[2, 1000:1100] = 0.0                                    # a drop-out
    whole, st, und = pm.run(v, c)
    assert (und == -1).all() and (st.off == 3000).all()
    parts, s = [], None
    for lo, hi in ((0, 1), (1, 777), (777, 2048), (2048, 3000)):
        t, s, _ = pm.run(v[:, lo:hi], c, s)
        parts.append(t)
    np.testing.assert_array_equal(np.concatenate(parts, axis=1).view(np.uint32), whole.view(np.uint32))
    for a, b in ((s.integ, st.integ), (s.phase, st.phase), (s.off, st.off), (s.fr, st.fr)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # one lane alone equals that lane of the batch
    t1, _, _ = pm.run(v[1], c)
    np.testing.assert_array_equal(t1.view(np.uint32), whole[1].view(np.uint32))


def carrier_of_locked_stream(oracle, n_blocks=24):
    p = oracle.mode_params(0)
    po = oracle.pipeline(0, 2)
    iq = oracle.synth_fm_u8(n_blocks * p.block_bytes // 2, seed=0x3D74)
    car = []
    for b in range(n_blocks):
        po.process(iq[b * p.block_bytes:(b + 1) * p.block_bytes])
        car.append(po.intermediate("carrier_filt"))
    return p, np.concatenate(car)


def test_model_follows_the_reference_loop(oracle):
    """The model on the oracle's pilot band-pass output of a locked synthetic stream (0.51 s) stays within 2 grid steps of
    the reference's fmPLL (oracle.fm_pll: atan2f / sinf / cosf of glibc), measured as
    test_gpu_parity.py::test_stereo_parallel_pll_matches_serial measures the parallel PLL against the serial one
    (|NCO difference| <= 2 * ncoScale * ulp(trigArg at the end) + 1e-6).  And it IS the fast form: its trigArg, put
    through glibc's cosf, leaves fmPLL's output somewhere after 0.1 s."""
    p, car = carrier_of_locked_stream(oracle)
    c = pm.coef(19e3, float(p.if_Fs))
    trig, st, und = pm.run(car, c)
    assert und == -1
    ref, ref_st = oracle.fm_pll(car, np.array([0, 0, 1, 0, 1, 0], np.float32), 19e3, float(p.if_Fs))
    u = 2.0 ** (math.floor(math.log2(c.w * len(car))) - 23)
    d = np.abs(pm.nco(trig, c) - ref[1:])
    print(f"model vs fm_pll over {len(car)} samples: NCO max |diff| {d.max():.3e} = {d.max() / u:.2f} ulp(trigArg)")
    assert d.max() <= 2 * 2 * u + 1e-6
    assert abs(float(st.off[0]) - float(ref_st[5])) == 0
    glibc_nco = oracle.libm("cosf", (trig * F32(2)).astype(F32))
    assert (glibc_nco[int(0.1 * p.if_Fs):] != ref[1 + int(0.1 * p.if_Fs):]).any()


def test_one_ulp_of_ki_leaves_the_nco_bound(oracle):
    """A loop constant one ulp off moves the trajectory by whole grid steps of trigArg: the NCO then leaves NCO_EPS, the
    bound the GPU tests hold the device's NCO to, by far -- the bound can tell such a change from the hardware cosine."""
    p, car = carrier_of_locked_stream(oracle, 8)
    c = pm.coef(19e3, float(p.if_Fs))
    base, _, _ = pm.run(car, c)
    bumped = pm.Coef(c.Kp, np.nextafter(c.Ki, F32(1)), c.w, c.nco_scale, c.phase_adjust)
    moved, _, _ = pm.run(car, bumped)
    d = np.abs(pm.nco(moved, c) - pm.nco(base, c))
    assert (moved != base).any() and d.max() > 20 * pm.NCO_EPS, d.max()
