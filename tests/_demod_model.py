"""Model of the fast FM discriminator (csrc/device_math.hpp: demod_fast / demod_fast_bounded), written from its documented
arithmetic in plain numpy float32.  It is the one definition the tests share; it neither calls nor links the product.

The arithmetic (every operation below is one IEEE float32 operation, rounded on its own -- no product is fused into a sum):

    ii = I*I   qq = Q*Q   den = ii + qq
    a = I*(Q - pq)   b = Q*(I - pi)   num = a - b
    sc = 2^64 where den < 2^-60, else 1            (so the reciprocal never sees a tiny operand)
    out = +0.0 where den == 0, else (num*sc) * rcp(den*sc)

rcp is the hardware reciprocal v_rcp_f32: within 1 ulp of 1/x, not correctly rounded, and the only operation here a host
cannot restate.  So the model comes in two forms:

  exact_given_rcp(parts, r)   the kernel's result BIT FOR BIT, given r = the device's own reciprocal of den*sc (read through
                              the rcp test hook);
  bracket(parts)              the three results for r in {RN(1/(den*sc)), its two float32 neighbours}: any reciprocal
                              within 1 ulp gives one of them.

demod_fast_bounded leaves the scaling out (sc = 1 always): the same bits wherever every operand is 0 or >= 2^-50 in
magnitude -- then den >= 2^-100 is far from the reciprocal's denormal range and num*2^64, den*2^64 are exact, and
rcp(x 2^64) = rcp(x) 2^-64 exactly (the reciprocal works on the mantissa; tests/test_gpu_demod_exact.py checks that too).

Denormals: the model KEEPS them (numpy float32 on the host does), as the kernels are built to (no flush-to-zero mode).
Only the reciprocal's own treatment of a denormal operand or result is the hardware's to say, and that is read from the
device, not modelled.  all_zero_or_normal() says whether a stream reaches any denormal intermediate at all; the pipeline's
streams never do: an IF sample is an integer times 2^-(s+7) (tests/_fe_model.py), so a nonzero den is >= 2^-2(s+7).
"""
from __future__ import annotations

import collections

import numpy as np

F32 = np.float32
THRESHOLD = F32(2.0 ** -60)      # den below this is scaled ...
FACTOR = F32(2.0 ** 64)          # ... by this
TINY = np.finfo(np.float32).tiny  # 2^-126, the smallest normal

Parts = collections.namedtuple("Parts", "num den sc ns ds ii qq dq di a b")


def _f32(*v):
    return tuple(np.ascontiguousarray(x, F32) for x in v)


def previous(I, Q, prev_i=0.0, prev_q=0.0):
    """(pi, pq): each sample's predecessor, the first one's being (prev_i, prev_q)."""
    I, Q = _f32(I, Q)
    return (np.concatenate([np.array([prev_i], F32), I[:-1]]), np.concatenate([np.array([prev_q], F32), Q[:-1]]))


def parts(I, Q, pi, pq):
    """num, den, sc, ns = num*sc and ds = den*sc exactly as demod_fast forms them (and the operations in between)."""
    I, Q, pi, pq = _f32(I, Q, pi, pq)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ii, qq = I * I, Q * Q
        den = ii + qq
        dq, di = Q - pq, I - pi
        a, b = I * dq, Q * di
        num = a - b
        sc = np.where(den < THRESHOLD, FACTOR, F32(1.0)).astype(F32)
        ns, ds = num * sc, den * sc
    return Parts(num, den, sc, ns, ds, ii, qq, dq, di, a, b)


def parts_bounded(I, Q, pi, pq):
    """The same for demod_fast_bounded: no scaling."""
    p = parts(I, Q, pi, pq)
    return p._replace(sc=np.ones_like(p.sc), ns=p.num, ds=p.den)


def exact_given_rcp(p, r):
    """The kernel's output bit for bit, r being the device's reciprocal of p.ds."""
    r = np.ascontiguousarray(r, F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        quot = p.ns * r
    return np.where(p.den == 0, F32(0.0), quot).astype(F32)


def rcp_rn(x):
    """RN(1/x) in float32.  Through float64 without a double rounding: 1/x of a 24-bit x is exact (a power of two) or at
    least 2^-49 (relative) away from every 25-bit midpoint, far more than the float64 quotient's 2^-53."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        return (1.0 / x.astype(np.float64)).astype(F32)


def rcp_candidates(x):
    """RN(1/x) and its two float32 neighbours, toward zero first: every reciprocal within 1 ulp is one of the three."""
    r = rcp_rn(x)
    away = np.copysign(F32(np.inf), r)
    return np.nextafter(r, F32(0.0)), r, np.nextafter(r, away)


def bracket(p):
    """The three candidates (num*sc) * r, r in rcp_candidates(den*sc); +0.0 where den == 0."""
    return tuple(exact_given_rcp(p, r) for r in rcp_candidates(p.ds))


def in_bracket(got, p):
    """Per sample: is got bit-equal to one of the bracket's candidates?"""
    g = np.ascontiguousarray(got, F32).view(np.uint32)
    ok = np.zeros(g.shape, bool)
    for c in bracket(p):
        ok |= g == c.view(np.uint32)
    return ok


def exact_divide(I, Q, pi, pq):
    """The exact-divide sibling (demod_exact, the reference's fmDemod): the same num and den, one IEEE divide."""
    p = parts(I, Q, pi, pq)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore", over="ignore"):
        quot = p.num / np.where(p.den == 0, F32(1.0), p.den)
    return np.where(p.den == 0, F32(0.0), quot).astype(F32)


def all_zero_or_normal(p):
    """True where every intermediate of the fast form -- the squares, the differences, the products, num, den, their scaled
    forms, the reciprocal and the three candidate quotients -- is zero or a normal finite number: no denormal, no overflow.
    On such a stream flushing and keeping denormals are the same arithmetic."""
    def ok(v):
        v = np.abs(np.asarray(v, F32))
        return (v == 0) | ((v >= TINY) & np.isfinite(v))
    good = np.ones(p.den.shape, bool)
    for v in (p.ii, p.qq, p.den, p.dq, p.di, p.a, p.b, p.num, p.ns, p.ds):
        good &= ok(v)
    nz = p.den != 0
    for r, c in zip(rcp_candidates(p.ds), bracket(p)):
        good &= ~nz | (ok(r) & ok(c))
    return good


# ---- mutants: what the model must tell apart (tests/test_demod_model_host.py) ------------------------------------------------
def fma32(x, y, z):
    """RN32(x*y + z) for float32 arrays: the product is exact in float64; the float64 sum rounds once more, which matters only
    where it lands on a float32 midpoint -- there the sign of the TwoSum residual decides."""
    x, y, z = (np.asarray(v, F32).astype(np.float64) for v in (x, y, z))
    pr = x * y
    s = pr + z
    bb = s - pr
    err = (pr - (s - bb)) + (z - bb)
    f = s.astype(F32)
    fix = np.flatnonzero(err != 0)
    if fix.size:
        sf, ff, ef = s[fix], f[fix], err[fix]
        other = np.nextafter(ff, np.where(sf > ff.astype(np.float64), F32(np.inf), F32(-np.inf)))
        tie = sf == (ff.astype(np.float64) + other.astype(np.float64)) / 2
        up = np.where(ef > 0, np.maximum(ff, other), np.minimum(ff, other))
        f[fix[tie]] = up[tie]
    return f


def mutant_num_fma(I, Q, pi, pq):
    """parts() with the numerator contracted: num = fma(I, Q - pq, -b)."""
    p = parts(I, Q, pi, pq)
    I, = _f32(I)
    num = fma32(I, p.dq, -p.b)
    return p._replace(num=num, ns=num * p.sc)


def mutant_den_fma(I, Q, pi, pq):
    """parts() with den contracted: den = fma(I, I, Q*Q)."""
    p = parts(I, Q, pi, pq)
    I, = _f32(I)
    den = fma32(I, I, p.qq)
    sc = np.where(den < THRESHOLD, FACTOR, F32(1.0)).astype(F32)
    return p._replace(den=den, sc=sc, ns=p.num * sc, ds=den * sc)


def ulps(got, want64):
    """|got - want| in units of the float32 ulp of want (want: float64, normal range)."""
    want64 = np.asarray(want64, np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(want64), float(TINY))))
    return np.abs(np.asarray(got, F32).astype(np.float64) - want64) / np.exp2(e - 23)
