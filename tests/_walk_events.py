"""The one-pole walk of csrc/onepole_walk.hpp in the device's order, plain numpy / Python: the lanes'
speculation, which the two filters' models share (`lanes`), and `verify`, a restatement of walk_verify for one row that counts
what it passes through.

`verify` is parametrised over the filter's step, step(g, y) -> y: sample g of the row behind the output y, on Python floats
that hold float32 values (_deemph_model.row_step, _highcut_model.row_step).  It scans windows of kScan * nt seams as the
workgroup's nt lanes do (lane tid looks at seams from + u nt + tid, u = 0 .. kScan - 1), takes the first miss, repairs as lane
0 does and resumes behind the repair.  Events, per row:

    miss                  segments walked again (the device's counter)
    met_inside            a repair that met the stored values inside its segment
    boundary_equal        a repaired segment ended without meeting them, and the next segment's start has the repaired end's bits
    chain_on              ... and the next segment's start differs: the repair walks on
    row_end               a repair that reached the row's end unmet (the last segment's end is rewritten)
    windows               scan passes
    miss_on_stride        a first miss at fm - from >= nt: found by a lane's u >= 1
    miss_in_later_window  a first miss found by a pass that `from = hi` entered
    chain_over_window     a repair that resumes behind its window: resume > hi
    miss_at_first_seam    fm == from
    miss_at_last_seam     fm == hi - 1

The models' parallel_rows are the definition of the result; this file is the definition of the order.  `drop` takes one line
out (DROPS): what a device without it would compute, for the test that shows the fixtures to notice."""
import math
import struct

import numpy as np

from _fir_model import fmaf

F32, F64 = np.float32, np.float64
FLT_MIN = 2.0 ** -126
K_SCAN, K_VERIFY_MAX, K_LANES = 8, 1024, 64          # kScan, kVerifyMax, kLanes (onepole_walk.hpp)
EVENTS = ("miss", "met_inside", "boundary_equal", "chain_on", "row_end", "windows", "miss_on_stride", "miss_in_later_window",
          "chain_over_window", "miss_at_first_seam", "miss_at_last_seam")
DROPS = ("stride", "next_window", "boundary_equal", "row_end")


def same(a, b):
    """equal bits, or both NaN: NaN payloads are not part of a definition"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same1(a, b):
    """same() on two Python floats"""
    if a == b:
        return a != 0.0 or math.copysign(1.0, a) == math.copysign(1.0, b)
    return a != a and b != b


def fmaf1(a, b, c):
    """fmaf on three Python floats that hold float32 values -> such a float.  a * b is exact in a double; float32(a * b + c) is
    right unless the double sum sits on a float32 midpoint or in the subnormal range (_fir_model._round_sum's rule): those go
    through _fir_model.fmaf."""
    s = a * b + c
    if s != s or s in (math.inf, -math.inf) or abs(s) < 2.0 ** -125 or \
            (struct.unpack("<Q", struct.pack("<d", s))[0] & 0x1FFFFFFF) == 0x10000000:
        return float(fmaf(np.array([a], F32), np.array([b], F32), np.array([c], F32))[0])   # (arrays: it repairs them in place)
    return float(F32(s))


def lanes(step, y0, n, W, L):
    """The segments kernel: one lane per (row, segment of L samples), all in step.  A lane starts W samples early from y = +0, or
    at sample 0 from the carried y0 [rows] where its warm-up would begin in front of the call.  step(r, g, y) -> y: rows r at
    samples g behind y, arrays of one shape.  -> (y [rows, n], start [rows, nseg], end [rows, nseg])."""
    rows = len(y0)
    nseg = (n + L - 1) // L
    r = np.arange(rows)[:, None]
    g0 = (np.arange(nseg) * L - W)[None, :].repeat(rows, 0)   # where each lane's warm-up would begin
    yp = np.where(g0 <= 0, np.asarray(y0, F32)[:, None], F32(0.0)).astype(F32)
    start = np.zeros((rows, nseg), F32)
    y = np.zeros((rows, n), F32)
    for j in range(W + L):
        g = g0 + j
        if j == W:
            start[:] = yp
        act = (g >= 0) & (g < n)
        gc = np.clip(g, 0, n - 1)
        ynew = step(r, gc, yp)
        yp = np.where(act, ynew, yp)
        if j >= W:
            rr, cc = np.nonzero(act)
            y[rr, g[rr, cc]] = yp[rr, cc]
    return y, start, yp.copy()


def verify_lanes(nseg):
    """lanes of a row's verify workgroup (walk::grid)"""
    return min((nseg + K_LANES - 1) // K_LANES * K_LANES, K_VERIFY_MAX)


def verify(step, y, start, end, n, L, nt=None, drop=()):
    """walk_verify for one row: y [n], start, end [nseg] as the lanes left them (not modified) ->
    (y, true end of the last segment, events: dict, found: [(from, hi, fm, resume)] per repair)."""
    with np.errstate(all="ignore"):
        return _verify(step, y, start, end, n, L, nt, drop)


def _verify(step, y, start, end, n, L, nt, drop):
    nseg = len(start)
    nt = verify_lanes(nseg) if nt is None else nt
    assert nseg == (n + L - 1) // L and nt >= 1 and all(d in DROPS for d in drop)
    bad = np.ones(nseg + 1, bool)                                # bad[c]: segment c's start is not segment c-1's end
    bad[1:nseg] = ~same(start[1:], end[:-1])
    bad[nseg] = False
    y, start, end = (np.asarray(v, F32).astype(F64).tolist() for v in (y, start, end))
    ev = dict.fromkeys(EVENTS, 0)
    found = []
    if "stride" in drop:
        offs = np.tile(np.arange(nt), K_SCAN)
    else:
        offs = (np.arange(K_SCAN)[:, None] * nt + np.arange(nt)[None, :]).reshape(-1)   # u * nt + tid
    frm, by_hi = 1, False
    while frm < nseg:
        hi = min(frm + K_SCAN * nt, nseg)
        ev["windows"] += 1
        c = frm + offs
        c = c[c < hi]
        hits = c[bad[c]]
        fm = int(hits.min()) if hits.size else nseg              # atomicMin over the lanes' finds
        if fm >= nseg:
            frm, by_hi = (nseg if "next_window" in drop else hi), True
            continue
        ev["miss_on_stride"] += fm - frm >= nt
        ev["miss_in_later_window"] += by_hi
        ev["miss_at_first_seam"] += fm == frm
        ev["miss_at_last_seam"] += fm == hi - 1
        c, yv = fm, end[fm - 1]
        while True:
            ev["miss"] += 1
            met = False
            for g in range(c * L, min(c * L + L, n)):
                yv = step(g, yv)
                if same1(yv, y[g]):
                    met = True
                    break
                y[g] = yv
            c += 1
            if met or c >= nseg:
                if met:
                    ev["met_inside"] += 1
                else:
                    ev["row_end"] += 1
                    if "row_end" not in drop:
                        end[c - 1] = yv
                break
            end[c - 1] = yv
            bad[c] = not same1(start[c], yv)
            if not bad[c] and "boundary_equal" not in drop:      # the next segment started from exactly this
                ev["boundary_equal"] += 1
                c += 1
                break
            ev["chain_on"] += 1
        ev["chain_over_window"] += c > hi
        found.append((frm, hi, fm, c))
        frm, by_hi = c, False
    return np.array(y, F64).astype(F32), F32(end[nseg - 1]), ev, found


def total(events):
    """the sum of several rows' events"""
    out = dict.fromkeys(EVENTS, 0)
    for e in events:
        for k in EVENTS:
            out[k] += int(e[k])
    return out


def table(ev):
    return ", ".join(f"{k} {ev[k]}" for k in EVENTS)
