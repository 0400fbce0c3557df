"""tests/_demod_model.py on the host: the model of the fast discriminator against the oracle's fmDemod, its error
contract in ulps, and its power to reject near-miss kernels (mutants).  No GPU: what the device adds -- the bits of its
reciprocal -- is tests/test_gpu_demod_exact.py's part."""
import numpy as np
import pytest

import _demod_model as dm

F = np.float32
N_STREAM = 200_000


def walk(amp, seed, n=N_STREAM, step=0.3):
    """A random-walk-phase trajectory of the given amplitude, quantised to 2^-32 (an IF sample is an integer times a power
    of two, tests/_fe_model.py): (I, Q) float32, exact."""
    rng = np.random.default_rng(seed)
    ph = np.cumsum(rng.standard_normal(n) * step)
    q = lambda v: (np.round(v * 2.0 ** 32) / 2.0 ** 32).astype(F)
    return q(amp * np.cos(ph)), q(amp * np.sin(ph))


@pytest.fixture(scope="module")
def strong():
    I, Q = walk(0.5, 1)
    pi, pq = dm.previous(I, Q)
    return I, Q, pi, pq, dm.parts(I, Q, pi, pq)


@pytest.fixture(scope="module")
def weak():
    I, Q = walk(2.0 ** -28, 2)
    pi, pq = dm.previous(I, Q)
    return I, Q, pi, pq, dm.parts(I, Q, pi, pq)


def rejected(true_parts, mutant_parts, r=None):
    """Fraction of samples on which the mutant's output (with the correctly rounded reciprocal unless r is given) is none of
    the three candidates the model allows."""
    r = dm.rcp_rn(mutant_parts.ds) if r is None else r
    return 1.0 - float(dm.in_bracket(dm.exact_given_rcp(mutant_parts, r), true_parts).mean())


def off_by_two(r):
    up = np.nextafter(np.nextafter(r, F(np.inf)), F(np.inf))
    down = np.nextafter(np.nextafter(r, F(0)), F(0))
    return up, down


def free_operands(rng, n):
    """Standard normals, then magnitudes swept 2^-80 .. 2^-20 (squares and den denormal or zero below 2^-63), then a block
    with exact zeros mixed in."""
    sets = [tuple(rng.standard_normal(n).astype(F) for _ in range(4))]
    e = rng.uniform(-80, -20, n)
    sets.append(tuple((rng.standard_normal(n) * np.exp2(e)).astype(F) for _ in range(4)))
    z = [(rng.standard_normal(n) * np.exp2(e)).astype(F) for _ in range(4)]
    for v in z:
        m = rng.random(n) < 0.2
        v[m] = rng.choice(np.array([0.0, -0.0], F), int(m.sum()))
    sets.append(tuple(z))
    return sets


def test_exact_divide_sibling_is_the_oracle(oracle):
    """The model's num and den with one IEEE divide = the oracle's fmDemod bit for bit, denormal products and den included: the
    model's statement of everything around the reciprocal is the reference's."""
    rng = np.random.default_rng(11)
    seen_denormal = False
    for I, Q, _, _ in free_operands(rng, 50_000):
        want, _, _ = oracle.fm_demod(I, Q, 0.25, -0.5)
        pi, pq = dm.previous(I, Q, 0.25, -0.5)
        got = dm.exact_divide(I, Q, pi, pq)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        p = dm.parts(I, Q, pi, pq)
        seen_denormal |= bool(((p.den > 0) & (p.den < dm.TINY)).any() and ((p.a != 0) & (np.abs(p.a) < dm.TINY)).any())
    assert seen_denormal


def test_bracket_is_within_four_ulp_of_the_ieee_quotient():
    """Every bracket candidate against RN(num/den) of the same num and den, in ulps of that quotient: <= 4.

    Derivation.  The outer candidates use a reciprocal up to 1.5 ulp(r) from 1/d (RN's half plus one step); ulp(r) <= 2^-23 |r|,
    so that is a relative 3 * 2^-24, and |x| < 2^24 ulp(x) makes it < 3 ulp of the quotient x (the worst case: significand of r
    near 1, of x near 2).  The product adds half an ulp, the IEEE divide it is compared with another half: 4.  Measured here:
    3.0 on the outer candidates, 1.0 on the centre one.  For a reciprocal within 1 ulp of 1/d (the hardware's contract) the same
    steps give 2 + 0.5 = 2.5 ulp of the true quotient at worst, about 1.5 on the average significand: what device_math.hpp says.
    Operands: standard normals, and den just below / num just below a power of two (the worst alignment)."""
    rng = np.random.default_rng(12)
    n = 400_000
    sets = [tuple(rng.standard_normal(n).astype(F) for _ in range(4))]
    # |z| just below 1 (1/den just above 1: the reciprocal's coarsest relative step), previous sample a quarter turn behind and
    # about twice as long: num / den just below 2
    th = rng.uniform(0, 2 * np.pi, n)
    rad = 1.0 - rng.uniform(0, 2.0 ** -12, n)
    I, Q = rad * np.cos(th), rad * np.sin(th)
    k = 2.0 - rng.uniform(0, 2.0 ** -10, n)
    sets.append(tuple(v.astype(F) for v in (I, Q, I + k * Q, Q - k * I)))
    worst = 0.0
    for I, Q, pi, pq in sets:
        p = dm.parts(I, Q, pi, pq)
        assert dm.all_zero_or_normal(p).all()
        nz = p.den != 0
        q = (p.num[nz] / p.den[nz]).astype(np.float64)
        for c in dm.bracket(p):
            live = q != 0
            u = dm.ulps(c[nz][live], q[live])
            worst = max(worst, float(u.max()))
            assert u.max() <= 4.0, float(u.max())
            assert not c[nz][~live].any()
    print(f"bracket vs IEEE quotient: worst {worst} ulp")
    assert worst >= 2.5          # the operands reach the regime the bound is about


def test_model_rejects_mutants_on_a_strong_stream(strong):
    """Amplitude about 0.5: a previous sample one too far back, a reciprocal 2 ulp off either way, and an fma-contracted
    numerator or den each leave the bracket on the stated share of samples."""
    I, Q, pi, pq, p = strong
    assert dm.all_zero_or_normal(p).all()
    pi2, pq2 = dm.previous(pi, pq)
    rates = dict(prev=rejected(p, dm.parts(I, Q, pi2, pq2)),
                 num_fma=rejected(p, dm.mutant_num_fma(I, Q, pi, pq)),
                 den_fma=rejected(p, dm.mutant_den_fma(I, Q, pi, pq)))
    for name, r in zip(("rcp_up2", "rcp_down2"), off_by_two(dm.rcp_rn(p.ds))):
        rates[name] = rejected(p, p, r)
    print(rates)
    assert rates["prev"] >= 0.999, rates
    assert rates["rcp_up2"] > 0.5 and rates["rcp_down2"] > 0.5, rates
    assert rates["num_fma"] >= 0.01 and rates["den_fma"] >= 0.01, rates
    assert rejected(p, p) == 0.0


def test_model_rejects_mutants_on_a_weak_stream(weak):
    """Amplitude 2^-28 on the 2^-32 grid: every product is exact, so a contraction changes nothing (why the strong stream is
    needed too).  The same stream 2^-8 lower puts den below 2^-60 on every sample: the scaled branch, the same bits as the
    unscaled form and as the stream it was scaled from."""
    I, Q, pi, pq, p = weak
    assert dm.all_zero_or_normal(p).all()
    pi2, pq2 = dm.previous(pi, pq)
    rates = dict(prev=rejected(p, dm.parts(I, Q, pi2, pq2)))
    for name, r in zip(("rcp_up2", "rcp_down2"), off_by_two(dm.rcp_rn(p.ds))):
        rates[name] = rejected(p, p, r)
    print(rates)
    assert rates["prev"] >= 0.9, rates
    assert rates["rcp_up2"] > 0.5 and rates["rcp_down2"] > 0.5, rates
    for mutant in (dm.mutant_num_fma, dm.mutant_den_fma):
        m = mutant(I, Q, pi, pq)
        assert np.array_equal(m.ns.view(np.uint32), p.ns.view(np.uint32)) and np.array_equal(m.ds.view(np.uint32), p.ds.view(np.uint32))
    k = F(2.0 ** -8)
    lo = dm.parts(I * k, Q * k, pi * k, pq * k)
    assert dm.all_zero_or_normal(lo).all()
    assert (lo.den[lo.den != 0] < dm.THRESHOLD).all() and (lo.sc[lo.den != 0] == dm.FACTOR).all() and (lo.den != 0).any()
    b = dm.parts_bounded(I * k, Q * k, pi * k, pq * k)
    for c, cl, cb in zip(dm.bracket(p), dm.bracket(lo), dm.bracket(b)):
        assert np.array_equal(c.view(np.uint32), cb.view(np.uint32)) and np.array_equal(cl.view(np.uint32), cb.view(np.uint32))


def test_degenerate_numerators_are_exact_zeros(strong, weak):
    """I*Q - Q*I (previous = (0, 0)): separately rounded products cancel to +0.0 and every candidate is the bit pattern of +0.0
    wherever den != 0; contracted, the same operands leave the product's rounding residue.  A constant IF gives 0."""
    for I, Q, _, _, _ in (strong, weak):
        z = np.zeros_like(I)
        p = dm.parts(I, Q, z, z)
        assert not p.num.view(np.uint32).any()
        for c in dm.bracket(p):
            assert not c.view(np.uint32).any()
        pc = dm.parts(I[:1].repeat(64), Q[:1].repeat(64), I[:1].repeat(64), Q[:1].repeat(64))
        for c in dm.bracket(pc):
            assert not c.any()
    I, Q = strong[0], strong[1]
    z = np.zeros_like(I)
    assert np.mean(dm.mutant_num_fma(I, Q, z, z).num != 0) > 0.5


def test_fma32_is_a_single_rounding():
    """The mutants' fma against exact rational arithmetic on operands that make the float64 sum inexact (ties included)."""
    from fractions import Fraction
    rng = np.random.default_rng(13)
    x = rng.standard_normal(2000).astype(F)
    y = rng.standard_normal(2000).astype(F)
    z = (rng.standard_normal(2000) * np.exp2(rng.integers(-40, 30, 2000))).astype(F)
    x[:4], y[:4] = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12)            # product 1 + 2^-11 + 2^-24: a float32 midpoint
    z[:4] = [F(0.0), F(2.0 ** -60), F(-2.0 ** -60), F(2.0 ** -23)]
    got = dm.fma32(x, y, z)
    for k in range(len(x)):
        exact = Fraction(float(x[k])) * Fraction(float(y[k])) + Fraction(float(z[k]))
        lo = F(float(exact))                                       # Python rounds a Fraction to float64 correctly; then
        cands = {float(np.nextafter(lo, F(-np.inf))), float(lo), float(np.nextafter(lo, F(np.inf)))}
        best = min(cands, key=lambda c: (abs(Fraction(c) - exact), int(np.float32(c).view(np.uint32)) & 1))
        assert float(got[k]) == best, (k, float(got[k]), best)
