"""What the GPU tests of the variable high-cut stage share (tests/test_gpu_highcut.py, tests/test_gpu_onepole_walk.py): the handle
and its model side by side, the six calls' meter records and inputs, and the comparison of one call."""
import numpy as np

import _highcut_model as hm
import _meters_model as mm
from _stage_cases import same_pcm, same_status

IF_FS, AUDIO_FS = 240000.0, 48000.0
CALLS = 6
BUILTIN = (hm.BUILTIN_W, hm.BUILTIN_L)
PSETS = dict(hm.PARAM_SETS, fast=dict(release=1.0))


def make(fmrx, N, ac, n, pset, shape=BUILTIN):
    p = hm.params(**PSETS[pset])
    if shape != BUILTIN:
        p.update(warmup=shape[0], segment=shape[1])
    return p, hm.control(p, IF_FS, AUDIO_FS), fmrx.HighCut(IF_FS, AUDIO_FS, N, ac, n, fmrx.HighCutParams(**p))


def records(c, N, calls=CALLS):
    """[calls][N] meter records: channel i walks the host tests' sequence i mod 5 (cycled, resets left out; channel 0 the walk
    0 -> partial -> full -> partial -> 0), every seventh the hand-made edge records"""
    seqs = [[r for r in s if r is not None] for s in hm.sequences(c).values()]
    edges = list(hm.hand_made_records().values())
    out = np.zeros((calls, N), mm.METER_DTYPE)
    for i in range(N):
        s = edges[i // 7:] + edges if i % 7 == 6 else seqs[i % len(seqs)]
        for k in range(calls):
            out[k, i] = s[k % len(s)]
    return out


def finite_even_rows(x):
    """A NaN or an infinity stays in a filter's state for as long as its pole is above 0, and the rest of the row says nothing:
    every other row keeps its +-0, subnormals and samples beyond +-2 but takes 2.5 for NaN and +-inf."""
    v = x.reshape(-1, x.shape[-1])
    v[::2] = np.where(np.isfinite(v[::2]), v[::2], np.float32(2.5))
    return x


def inputs(kind, rng, N, ac, n, calls=CALLS):
    """[calls][N, ac, n]: seeded noise with +-0, NaN, +-inf and values beyond +-2, or the three fixed inputs, row r taking
    input r mod 3, cut into the calls one behind the other"""
    if kind == "noise":
        return [finite_even_rows(hm.random_rows(rng, N, ac, n)) for _ in range(calls)]
    d = hm.fixed_inputs(calls * n)
    rows = np.stack([d[k] for k in ("audio", "audio->silence", "impulse")])
    pick = np.arange(N * ac) % 3
    return [np.ascontiguousarray(rows[pick, k * n:(k + 1) * n]).reshape(N, ac, n) for k in range(calls)]


class Model:
    """the model's side of a handle: status rows, filter state, the diagnostics' counts"""

    def __init__(self, c, N, ac, shape):
        self.c, self.N, self.ac, self.shape = c, N, ac, shape
        self.status, self.state, self.segments, self.missed = hm.fresh(N), np.zeros(N * ac, np.float32), 0, 0

    def call(self, recs, audio, counted=True):
        self.status = hm.step_all(self.c, recs, self.status)
        y, self.state, missed, segs = hm.apply(self.c, self.status, audio, self.state, *self.shape)
        if counted:
            self.segments, self.missed = self.segments + segs, self.missed + missed
        return y

    def reset(self, ch):
        self.status[ch] = hm.fresh()
        self.state[ch * self.ac:(ch + 1) * self.ac] = 0


def check_call(oracle, out, hc, model, want, wrap, f32, pcm):
    same_status(hc.status(), model.status, hm.STATUS_DTYPE.names)
    if f32:
        ok = hm.same(out["audio"], want)
        assert ok.all(), (np.argwhere(~ok)[:5], out["audio"][~ok][:5], want[~ok][:5])
    if pcm:
        same_pcm(oracle, out["pcm16"], want, wrap)
    assert hc.diagnostics() == {"segments": model.segments, "missed": model.missed}
