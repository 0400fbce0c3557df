"""A plain numpy model of the parallel-in-time form of the stereo PLL (csrc/kernels_pll.hip: pll_lti_chunks_kernel,
pll_segments_kernel, pll_repair_kernel), on top of the fast step of tests/_pll_model.py.  Vectorised over segments: a walk is
64 steps of array arithmetic.

  lti_records   the chunk kernel in float64, in the kernel's order of operations (the file is built under fp contract(off),
                so every product and sum below is rounded as there): per 64-sample chunk its zero-state response to its own
                staircase, its climb (with the look into the next chunk's first sample), the exclusive prefix of the climbs
                inside its workgroup of 64 chunks, and the workgroup totals.  Climbs are multiples of 1/2: their sums are exact
                in any order.
  lti_start     lti_start_setup + lti_start_state: the locked loop's (integ, phase) in front of sample 64 i as float32, from the
                20 chunks behind it, the block's true state substituted near its start, i == 0 the state itself.
  walk          the fast step over whole segments from (integ, phase) at trigOffset off, fr = reduce(float(w off + phase)):
                what a lane runs in its own segment, and what the serial recurrence continues with from a segment's end
                (a step's fr IS the reduced float32 trigArg = float(w off + phase) of the state it leaves).
  tolerances    pll_phase_tol, pll_integ_tol in float32 as written; phase_dist = pll_phase_dist.
  simulate      the whole scheme on the model (lanes from lti_start, warm-up, judge, repair rounds as the kernels order them),
                with the repair rule chosen.  The kernels' rule: after a walk the successor is judged anew -- one still in its
                own lane by its warm-up start to the tolerances, one that was itself walked by the state it was walked from,
                BIT FOR BIT (it stays only if its predecessor's end came out the same).  The rule before (`lane_basis=True`):
                always by the lane's warm-up start, which a walked segment's outputs no longer come from."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import _pll_model as pm

F32, F64 = np.float32, np.float64
CHUNK = 64                  # kLtiChunk
LTI_TERMS = 20              # kLtiTerms
TWO_PI = 6.28318530717958647692
TOL_PHASE, TOL_INTEG = F32(1e-2), F32(1e-4)       # kPllTolPhase, kPllTolInteg
INTEG_TOL_ULPS = {False: F32(2.0), True: F32(6.0)}   # PllCoef::integ_tol_ulps; kPllIntegTolUlpsLti
RESET = np.array([0, 0, 1, 0, 1, 0], F32)


@dataclass
class Lti:
    """make_coef's linear system: s' = A s + B x in (phase, integrator) / 2 pi; Q = A^64, G = 64 steps' response to x = 1."""
    a00: float
    a01: float
    a10: float
    a11: float
    b0: float
    b1: float
    q: tuple
    g: tuple
    f: float


def lti_of(c: pm.Coef) -> Lti:
    Kp, Ki = float(c.Kp), float(c.Ki)
    a00, a01, a10, a11, b0, b1 = 1.0 - Kp - Ki, 1.0, -Ki, 1.0, Kp + Ki, Ki
    g0 = g1 = 0.0
    q00, q01, q10, q11 = 1.0, 0.0, 0.0, 1.0
    for _ in range(CHUNK):
        g0, g1 = a00 * g0 + a01 * g1 + b0, a10 * g0 + a11 * g1 + b1
        q00, q01, q10, q11 = a00 * q00 + a01 * q10, a00 * q01 + a01 * q11, a10 * q00 + a11 * q10, a10 * q01 + a11 * q11
    return Lti(a00, a01, a10, a11, b0, b1, (q00, q01, q10, q11), (g0, g1), c.w * pm.INV_2PI)


def lti_step(m: Lti, phi, iota, x):
    p = m.a00 * phi + m.a01 * iota + m.b0 * x
    iota = m.a10 * phi + m.a11 * iota + m.b1 * x
    return p, iota


def lti_records(signs, c: pm.Coef, n: int, look_ahead=True) -> dict:
    """signs[n]: in[k] > 0.  look_ahead=False: a climb that ignores the next chunk's first sample (a sensitivity check)."""
    pos = np.asarray(signs, bool)[:n]
    m = lti_of(c)
    nchunk = n // CHUNK + 1
    # a sample at or past n takes the last sign seen (pn = k < n ? vn > 0 : pos)
    P = np.concatenate([pos, np.full(nchunk * CHUNK + 1 - n, pos[n - 1])])
    k0 = np.arange(nchunk) * CHUNK
    phi, iota, dT = np.zeros(nchunk), np.zeros(nchunk), np.zeros(nchunk)
    for j in range(CHUNK):
        phi, iota = lti_step(m, phi, iota, dT - m.f * j)
        if j + 1 < CHUNK or look_ahead:
            dT = dT + np.where(P[k0 + j + 1] != P[k0 + j], 0.5, 0.0)
    nwg = (nchunk + 63) // 64
    d = np.zeros(nwg * 64)
    d[:nchunk] = dT
    d = d.reshape(nwg, 64)
    pre = (np.cumsum(d, axis=1) - d).reshape(-1)[:nchunk]
    return {"phi": phi, "iota": iota, "pre": pre, "dT": dT, "wgtot": d.sum(axis=1), "in0_pos": bool(pos[0]), "lti": m, "w": c.w,
            "nchunk": nchunk}


def lti_start(state, rec: dict, i, terms=LTI_TERMS):
    """(integ, phase) float32 arrays in front of sample 64 i (i: chunk indices, < nchunk)."""
    i = np.atleast_1d(np.asarray(i, np.int64))
    m: Lti = rec["lti"]
    q00, q01, q10, q11 = m.q
    g0, g1 = m.g
    st = np.asarray(state, F32)
    phi0, iota0, off0 = float(st[1]) * pm.INV_2PI, float(st[0]) * pm.INV_2PI, float(st[5])
    trig0 = F32(rec["w"] * off0 + float(st[1]))
    th0 = float(trig0) * pm.INV_2PI
    T0 = float(np.rint(th0)) if rec["in0_pos"] else float(np.rint(th0 - 0.5)) + 0.5
    wgbase = np.concatenate([[0.0], np.cumsum(rec["wgtot"])])          # climb of all workgroups in front of workgroup w
    p, q = np.zeros(len(i)), np.zeros(len(i))
    for t in range(terms):
        jj = i - (terms - t)
        j = np.maximum(jj, 0)
        base = ((T0 + wgbase[j // 64] + rec["pre"][j]) - m.f * (off0 + (j * CHUNK).astype(F64))) - phi0
        r0 = rec["phi"][j] + base * g0
        r1 = rec["iota"][j] + base * g1
        first = jj == 0
        p = np.where(first, 0.0, p)
        q = np.where(first, iota0, q)
        np_ = q00 * p + q01 * q + r0
        nq = q10 * p + q11 * q + r1
        p = np.where(jj >= 0, np_, p)
        q = np.where(jj >= 0, nq, q)
    p = np.where(i == 0, 0.0, p)
    q = np.where(i == 0, iota0, q)
    return (q * TWO_PI).astype(F32), ((phi0 + p) * TWO_PI).astype(F32)


def fr_of(off, phase, c: pm.Coef) -> np.ndarray:
    """fr of a lane that starts at trigOffset off with phase estimate phase: reduce(float(w off + phase))."""
    t = (c.w * np.asarray(off, F32).astype(F64) + np.asarray(phase, F32).astype(F64)).astype(F32)
    rev = t.astype(F64) * pm.INV_2PI
    return (rev - np.rint(rev)).astype(F32)


def walk(start_integ, start_phase, off, v, c: pm.Coef):
    """v [S, m] (or [m]): S segments' samples; start_integ, start_phase, off [S] float32: the state in front of them.
    Returns (trig [S, m], end_integ [S], end_phase [S], und [S]: first undetermined step or -1)."""
    v = np.atleast_2d(np.asarray(v, F32))
    integ = np.atleast_1d(np.asarray(start_integ, F32)).copy()
    phase = np.atleast_1d(np.asarray(start_phase, F32)).copy()
    off = np.atleast_1d(np.asarray(off, F32)).copy()
    st = pm.State(integ, phase, off, fr_of(off, phase, c))
    trig, end, und = pm.run(v, c, st)
    return trig, end.integ, end.phase, und


def trig_ulp(state, n: int, c: pm.Coef) -> np.float32:
    """pll_trig_ulp: 2^(e - 23) of the float32 trigArg the block ends on."""
    top = np.array(c.w * (float(F32(state[5])) + float(n)), F32)
    return (top.view(np.uint32) & np.uint32(0x7F800000)).view(F32)[()] * F32(1.1920929e-7)


def tolerances(state, n: int, c: pm.Coef, lti: bool):
    """(tol_phase, tol_integ) float32: base + 2 ulp(trigArg at the block's end); base + ulps * Ki * ulp."""
    u = trig_ulp(state, n, c)
    return F32(TOL_PHASE + F32(F32(2.0) * u)), F32(TOL_INTEG + F32(F32(INTEG_TOL_ULPS[bool(lti)] * c.Ki) * u))


def phase_dist(a, b) -> np.ndarray:
    """pll_phase_dist: |a - b| modulo 2 pi, float32 as written."""
    d = (np.asarray(a, F32) - np.asarray(b, F32)).astype(F32)
    turns = np.rint((d * F32(pm.INV_2PI)).astype(F32)).astype(F32)
    return np.abs((d - (F32(TWO_PI) * turns).astype(F32)).astype(F32))


def merged(b_integ, b_phase, e_integ, e_phase, tol):
    return (phase_dist(b_phase, e_phase) <= tol[0]) & (np.abs((np.asarray(b_integ, F32) - np.asarray(e_integ, F32)).astype(F32)) <= tol[1])


def segments_of(v, L):
    """The block as [nfull, L] whole segments and the ragged last one (or None)."""
    n = len(v)
    nfull = n // L
    return np.asarray(v[:nfull * L], F32).reshape(nfull, L), (np.asarray(v[nfull * L:], F32) if n % L else None)


def walk_all(integ, phase, off0, v, L, c):
    """walk() of every segment of the block v (the ragged last one too) from per-segment (integ, phase):
    trig [n], end_integ, end_phase, und [nseg]."""
    full, tail = segments_of(v, L)
    nfull = len(full)
    off = (F32(off0) + (np.arange(nfull + (tail is not None)) * L).astype(F32)).astype(F32)
    t, ei, ep, u = walk(integ[:nfull], phase[:nfull], off[:nfull], full, c)
    trig = [t.reshape(-1)]
    if tail is not None:
        t2, ei2, ep2, u2 = walk(integ[nfull:], phase[nfull:], off[nfull:], tail, c)
        trig.append(t2.reshape(-1))
        ei, ep, u = np.concatenate([ei, ei2]), np.concatenate([ep, ep2]), np.concatenate([u, u2])
    return np.concatenate(trig), ei, ep, u


def simulate(v, state, c: pm.Coef, W=64, fr0=None, lane_basis=False):
    """The scheme with the linear start (pll_start 1, L = 64) on the model: lanes from lti_start W samples early (W a multiple
    of 64), the judge of every seam, the repair rounds of pll_repair_kernel (a round = every flagged segment whose predecessor
    is not flagged; after a walk the successor is judged anew).  A re-walked segment takes the model's exact fr (the device
    rebuilds it with atan2f).  fr0: fr of the incoming state (default: of its trigArg).
    Returns dict: end [nseg, 2], basis [nseg, 2], walks [nseg], repaired, und [nseg], tol, stale (segments whose basis is
    outside the tolerances of their predecessor's final end)."""
    v = np.asarray(v, F32)
    n, L = len(v), CHUNK
    st = np.asarray(state, F32)
    nseg = (n + L - 1) // L
    rec = lti_records(v > 0, c, n)
    a = np.arange(nseg) * L
    k0 = np.where(a > W, a - W, 0)
    integ, phase = lti_start(st, rec, k0 // CHUNK)
    integ[k0 == 0], phase[k0 == 0] = st[0], st[1]
    off = (st[5] + k0.astype(F32)).astype(F32)
    fr = fr_of(off, phase, c)
    if fr0 is not None:
        fr[k0 == 0] = F32(fr0)
    und = np.full(nseg, -1, np.int64)
    # warm-up: lanes step while they are in front of their segment
    vp = np.concatenate([v, np.zeros(L, F32)])
    for j in range(int((a - k0).max())):
        act = k0 + j < a
        idx = np.flatnonzero(act)
        _, s2, _ = pm.run(vp[(k0 + j)[idx]].reshape(-1, 1), c, pm.State(integ[idx], phase[idx], off[idx], fr[idx]))
        integ[idx], phase[idx], off[idx], fr[idx] = s2.integ, s2.phase, s2.off, s2.fr
    basis = np.stack([integ, phase], axis=1).astype(F32)
    full, tail = segments_of(v, L)
    nfull = len(full)
    _, se, u = pm.run(full, c, pm.State(integ[:nfull], phase[:nfull], off[:nfull], fr[:nfull]))
    end = np.zeros((nseg, 2), F32)
    end[:nfull, 0], end[:nfull, 1], und[:nfull] = se.integ, se.phase, u
    if tail is not None:
        _, se, u = pm.run(tail.reshape(1, -1), c, pm.State(integ[nfull:], phase[nfull:], off[nfull:], fr[nfull:]))
        end[nfull:, 0], end[nfull:, 1], und[nfull:] = se.integ, se.phase, u
    tol = tolerances(st, n, c, True)
    bad = np.zeros(nseg, bool)
    bad[1:] = ~merged(basis[1:, 0], basis[1:, 1], end[:-1, 0], end[:-1, 1], tol)
    lane = basis.copy()
    walks = np.zeros(nseg, np.int64)
    repaired = 0
    while True:
        todo = np.flatnonzero(bad[1:] & ~bad[:-1]) + 1
        if len(todo) == 0:
            break
        for s in todo:
            lo, hi = s * L, min(n, s * L + L)
            basis[s] = end[s - 1]
            _, ei, ep, u = walk(end[s - 1, 0], end[s - 1, 1], F32(st[5] + F32(lo)), v[lo:hi], c)
            end[s], und[s] = (ei[0], ep[0]), u[0]
            walks[s] += 1
            repaired += 1
            bad[s] = False
            if s + 1 < nseg:
                if walks[s + 1] and not lane_basis:         # walked from this segment's earlier end: the same bits, or again
                    bad[s + 1] = bool((basis[s + 1].view(np.uint32) != end[s].view(np.uint32)).any())
                else:
                    bad[s + 1] = not merged(lane[s + 1, 0], lane[s + 1, 1], end[s, 0], end[s, 1], tol)
    stale = np.flatnonzero(~merged(basis[1:, 0], basis[1:, 1], end[:-1, 0], end[:-1, 1], tol)) + 1
    gap = phase_dist(basis[1:, 1], end[:-1, 1])
    return {"end": end, "basis": basis, "walks": walks, "repaired": repaired, "und": und, "tol": tol, "stale": stale,
            "stale_gap": float(gap[stale - 1].max()) if len(stale) else 0.0}


# ---- the crafted inputs of tests/test_gpu_pll_parallel.py (and the host test that vouches for them) ----
def tone(n, seed=1, noise=0.02, phase0=0.3, jump_at=None, jump=0.0, start=0):
    """A 19 kHz pilot at 240 kHz with white noise, float32; sample k stands at stream position start + k."""
    rng = np.random.default_rng(seed)
    k = np.arange(start, start + n, dtype=F64)
    ph = 2 * math.pi * 19e3 / 240e3 * k + phase0
    if jump_at is not None:
        ph[jump_at:] += jump
    return (np.cos(ph) + noise * rng.standard_normal(n)).astype(F32)


def with_dropouts(v, gaps, seed=7):
    """(start, length) stretches replaced by unit white noise."""
    rng = np.random.default_rng(seed)
    v = v.copy()
    for lo, m in gaps:
        v[lo:lo + m] = rng.standard_normal(m).astype(F32)
    return v


def no_pilot(n, seed=3):
    return np.random.default_rng(seed).standard_normal(n).astype(F32)


N_FIX = 64 * 200                                   # samples of a fixture
# drop-outs of 3, 40 and 400 samples, two of each; places and noise seeded (114) so that simulate() walks 18 segments twice
# from the reset state and from a locked one
DROPOUTS = [(2247, 400), (3021, 40), (3222, 400), (6137, 3), (9288, 3), (11065, 40)]
ZERO_RUN = (6000, 150)                             # exact zeros: the wave-uniform general step
EXEMPT_CAP = 0.01                                  # share of a call's segments that may hold an undetermined step


def fixtures(start=0, n=N_FIX) -> dict:
    """name -> (samples, has_zeros), the stream standing at position `start` (a first call's length or 0)."""
    clean = tone(n, seed=2, start=start)
    zeros = clean.copy()
    zeros[ZERO_RUN[0]:ZERO_RUN[0] + ZERO_RUN[1]] = 0.0
    return {"tone": (clean, False),
            "jump": (tone(n, seed=2, start=start, jump_at=n // 2 + 17, jump=2.0), False),
            "dropouts": (with_dropouts(clean, DROPOUTS, seed=114), False),
            "zeros": (zeros, True),
            "no_pilot": (no_pilot(n), False)}
