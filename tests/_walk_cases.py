"""What the tests of the one-pole walk feed (tests/test_walk_model_host.py, tests/test_gpu_onepole_walk.py): lane shapes, row
lengths by segment count, the rows' inputs, and the models' results for a case -- serial, parallel and, row by row, the
device's order with its events (tests/_walk_events.py).

Segment counts: a row's verify workgroup has min(ceil64(nseg), 1024) lanes and scans windows of 8 times as many seams, so 64 /
65 are the last row of one wave and the first of two, 1024 / 1025 the last row with a lane per segment and the first whose
workgroup is capped (longer rows have seams on a lane's second and later strides), 8193 the last one-window row (seams 1 ..
8192), 8194 the first with a second window, 16 390 a row with a third."""
import numpy as np

import _deemph_model as m
import _highcut_cases as hcc
import _highcut_model as hm
import _walk_events as we

F32 = np.float32
FS = 48000.0
SHAPES = [(0, 1), (0, 4), (1, 3), (2, 2), (8, 2), (256, 1), (100, 7), (40, 16), (8, 40), (40, 24), (31, 33), (33, 31), (32, 32)]
NSEGS = (1, 2, 64, 65, 1024, 1025, 8193, 8194, 16390)
N_LIMIT = 40000                     # samples per row, exclusive
LONG = 8193                         # from this many segments on: LONG_KINDS as rows, no more
KINDS = ("audio", "audio->silence", "impulse", "flush 4e-38", "flush 1e-37", "late Inf/NaN", "edge: last seam", "edge: first seam",
         "edge: chain across", "zeros", "subnormals")
QUIET = ("zeros", "subnormals")     # rows that must not miss
LONG_KINDS = ("edge: last seam", "edge: first seam", "edge: chain across", "late Inf/NaN", "flush 1e-37", "flush 4e-38", "audio->silence",
              "subnormals")
ROWS_MAX = 70
IMPULSE = F32(1e30)                 # dies away over 551 samples at 75 us, 48 kHz


def shape_id(s):
    return f"W{s[0]}L{s[1]}"


def lengths(L):
    """[(nseg, n)]: every segment count whose rows stay under N_LIMIT, with n a multiple of L (up to 1025 segments, and where
    L = 1) and once ragged (where L > 1)"""
    out = []
    for nseg in NSEGS:
        if nseg * L >= N_LIMIT:
            continue
        if nseg < LONG or L == 1:
            out.append((nseg, nseg * L))
        if L > 1:
            out.append((nseg, (nseg - 1) * L + 1 + nseg % (L - 1)))
    assert all((n + L - 1) // L == nseg for nseg, n in out)
    return out


def first_window(nseg):
    """hi of the first scan pass"""
    return min(1 + we.K_SCAN * we.verify_lanes(nseg), nseg)


def edge_seams(W, L, nseg):
    """The seams the three window-edge rows aim their first miss at: the last seam of the first window; the first seam of the
    second window (a one-window row: the earliest seam that can miss -- a lane whose warm-up begins at or in front of sample 0
    starts from the carried state and is exact); a few seams in front of the window's edge (a one-window row: mid-row), from
    where the repairs chain across it."""
    hi, lowest = first_window(nseg), W // L + 1
    return {"edge: last seam": hi - 1, "edge: first seam": hi if hi < nseg else lowest,
            "edge: chain across": max(lowest, hi - 6 if hi < nseg else nseg // 2)}


def _fixed(n):
    d = m.fixed_inputs(max(n, 4096))
    audio = d["audio"][:n].copy()
    silence = audio.copy()
    silence[min(1500, 3 * n // 8):] = 0
    impulse = d["impulse"][:n].copy()
    if n <= 700:
        impulse[n // 6] = IMPULSE
    return {"audio": audio, "audio->silence": silence, "impulse": impulse}


def row(kind, W, L, n, seed=0):
    """One row of `kind` -> (x [n], carried state (x_prev, y_prev))"""
    nseg = (n + L - 1) // L
    rng = np.random.default_rng([KINDS.index(kind), seed])
    carried = (0.25 * rng.standard_normal(2)).astype(F32)
    zero = np.zeros(2, F32)
    if kind in ("audio", "audio->silence", "impulse"):
        return np.roll(_fixed(n)[kind], 37 * seed), carried
    if kind.startswith("flush"):
        return (float(kind.split()[1]) * rng.standard_normal(n)).astype(F32), carried
    if kind == "zeros":
        return np.zeros(n, F32), zero
    if kind == "subnormals":
        x = (1e-40 * rng.standard_normal(n)).astype(F32)
        assert np.all(np.abs(x) < 2.0 ** -126)
        return x, zero
    if kind == "late Inf/NaN":
        # +Inf, -Inf (their sum: NaN) and NaN: from the +Inf on no lane's start equals the true state and no repair meets the
        # stored values, to the row's end.  In the rows with a third window the chain starts behind seam 8193.
        x = (0.1 * rng.standard_normal(n)).astype(F32)
        seam = LONG + 57 if nseg > LONG + 300 else nseg // 3
        at = [seam * L, (seam + 100) * L + L // 2, (seam + 200) * L] if nseg > 600 else [n // 3, n // 2, 2 * n // 3]
        if W < 64:
            x[:at[0]] = 0                        # a short warm-up misses on noise everywhere: silence in front of the +Inf
            carried = zero
        if n >= 6:
            x[at[0]], x[at[1]], x[at[2]] = np.inf, -np.inf, np.nan
        return x, carried
    # the window-edge rows: one impulse at the last sample that segment s - 1's lane still sees and segment s's does not
    # (s L - W - 1), on `audio` where the shape's warm-up reaches the true bits on it, else on digital silence
    x = _fixed(n)["audio"] if W >= 256 else np.zeros(n, F32)
    at = edge_seams(W, L, nseg)[kind] * L - W - 1 + seed
    if 0 <= at < n:
        x[at] = IMPULSE
    return x, (carried if W >= 256 else zero)


def rows_of(nseg):
    """rows of a de-emphasis case: 70 where rows change inside a workgroup of the segments kernel (nseg % 64 != 0), one of
    each kind elsewhere (the models' time goes with rows x samples)"""
    return len(LONG_KINDS) if nseg >= LONG else ROWS_MAX if nseg % 64 else len(KINDS)


def kinds_of(nseg, rows=None, seed=0):
    k = LONG_KINDS if nseg >= LONG else KINDS
    rows = rows_of(nseg) if rows is None else rows
    return [(k[i % len(k)], seed + i // len(k)) for i in range(rows)]


def inputs(W, L, n, rows=None, seed=0):
    """-> (x [rows, n], state [rows, 2], the rows' kinds): the kinds in turn, later copies with another seed or rotated"""
    ks = kinds_of((n + L - 1) // L, rows, seed)
    made = [row(k, W, L, n, s) for k, s in ks]
    return np.stack([a for a, _ in made]), np.stack([b for _, b in made]), [k for k, _ in ks]


def device_order(x, state, spec, p, b0, L, rows=None, drop=()):
    """_walk_events.verify on the first `rows` rows of a de-emphasis case -> (y, state, [events], [found])"""
    rows = len(x) if rows is None else rows
    ys, st, evs, fnd = [], [], [], []
    for r in range(rows):
        y, e, ev, found = we.verify(m.row_step(x[r], state[r, 0], p, b0), spec[0][r], spec[1][r], spec[2][r], x.shape[1], L, drop=drop)
        ys.append(y)
        st.append([x[r, -1], e])
        evs.append(ev)
        fnd.append(found)
    return np.stack(ys), np.array(st, F32), evs, fnd


def deemph_case(W, L, n, p, b0, rows=None, event_rows=len(KINDS)):
    """One (shape, n) of the de-emphasis sweep: the inputs, the model's parallel walk on all rows (y, state_out, missed per
    row) and the device's order on the first event_rows of them (dev_y, dev_state, events, found)"""
    x, state, kinds = inputs(W, L, n, rows)
    spec = m.speculate(x, p, b0, state, W, L)
    y, state_out, missed, checked = m.parallel_rows(x, p, b0, state, W, L, spec=spec)
    R = min(event_rows, len(x))
    dev_y, dev_state, events, found = device_order(x, state, spec, p, b0, L, R)
    return dict(W=W, L=L, n=n, nseg=(n + L - 1) // L, x=x, state=state, kinds=kinds, spec=spec, y=y, state_out=state_out, missed=missed,
                checked=checked, dev_y=dev_y, dev_state=dev_state, events=events, found=found)


# ---- the high-cut's cases --------------------------------------------------------------------------------------------------
def highcut_cases():
    """Every shape at 65, 1025 and 8194 segments (where the row stays under N_LIMIT; the ragged length where L > 1), each with
    one of N in {1, 3, 35} x ac in {1, 2} (35 channels at 65 segments only, 8194 segments with at most 3 rows: the model's time
    goes with rows x samples), in place or not, f32 / PCM / both, wrap or saturate in turn."""
    out = []
    combos = {65: [(35, 2), (1, 1), (3, 2), (35, 1), (1, 2), (3, 1)], 1025: [(3, 1), (1, 2), (1, 1), (3, 2)], 8194: [(1, 2), (3, 1), (1, 1)]}
    outputs = [(True, True), (True, False), (False, True)]
    for W, L in SHAPES:
        for nseg in (65, 1025, 8194):
            ns = [n for s, n in lengths(L) if s == nseg]
            if not ns:
                continue
            i = len(out)
            N, ac = combos[nseg][SHAPES.index((W, L)) % len(combos[nseg])]
            out.append(dict(W=W, L=L, nseg=nseg, n=ns[-1], N=N, ac=ac, in_place=i % 2 == 0, f32=outputs[i % 3][0], pcm=outputs[i % 3][1],
                            wrap=i % 4 < 2))
    return out


def highcut_id(c):
    return (f"W{c['W']}L{c['L']}-nseg{c['nseg']}-{c['N']}x{c['ac']}-{'inplace' if c['in_place'] else 'outofplace'}-"
            f"{'f32' if c['f32'] else ''}{'pcm' if c['pcm'] else ''}-{'wrap' if c['wrap'] else 'sat'}")


def highcut_inputs(c, call):
    """[N, ac, n] of call `call`: the de-emphasis' kinds row by row, NaN and the infinities swapped for 2.5 on every other row"""
    x, _, kinds = inputs(c["W"], c["L"], c["n"], c["N"] * c["ac"], seed=call)
    return hcc.finite_even_rows(np.ascontiguousarray(x).reshape(c["N"], c["ac"], c["n"])), kinds


class HighcutWalk(hcc.Model):
    """_highcut_cases.Model whose call also walks the first rows in the device's order: .last holds that walk's rows, states
    and events next to the model's rows, states and misses"""

    def call(self, recs, audio, counted=True, event_rows=len(KINDS)):
        self.status = hm.step_all(self.c, recs, self.status)
        a = np.asarray(audio, F32)
        N, ac, n = a.shape
        x = a.reshape(N * ac, n)
        p0, p1, p_max = np.repeat(self.status["p0"], ac), np.repeat(self.status["p1"], ac), self.c["p_max"]
        W, L = self.shape
        spec = hm.speculate(x, p0, p1, p_max, self.state, W, L)
        y, st, missed, segs = hm.parallel_rows(x, p0, p1, p_max, self.state, W, L, spec=spec)
        R = min(event_rows, len(x))
        walks = [we.verify(hm.row_step(x[r], p0[r], p1[r], p_max), spec[0][r], spec[1][r], spec[2][r], n, L) for r in range(R)]
        self.last = dict(x=x, p0=p0, p1=p1, state_in=self.state, y=y, state=st, missed=missed, dev_y=np.stack([w[0] for w in walks]),
                         dev_state=np.array([w[1] for w in walks], F32), events=[w[2] for w in walks])
        self.state = st
        if counted:
            self.segments, self.missed = self.segments + segs, self.missed + int(missed.sum())
        return y.reshape(a.shape)
