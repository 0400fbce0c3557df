"""Calls and banks whose buffers reach past 2^32 bytes (tests/_large_calls.py says how a result of that size is checked).

The project advertises shapes the rest of the suite never reaches: bench.py's step is 2.1 GB of I/Q in one call, its bank
legs are 6.7 GB of input slots.  A `long` that became an `int`, a 32-bit voffset, a buffer resource whose num_records
was cut, a pitch product in 32 bits, a grid dimension above what the launch accepts or a ctypes signature that truncates
a size would show nowhere else.  Every case here moves >= 2^32 + 64 MiB through the buffer named in its docstring:

  A  Pipeline(0, 1), the fused mono kernel (straight-line, general and tail paths); f32 + PCM, PCM only wrap / saturate
  B  Pipeline(1, 1), intermediates kept: fe_mfma_kernel, audio_fir_kernel, hist_update; the interleaved IF crosses too
  C  Pipeline(0, 1), fe_variant valu: fe_demod_kernel + audio_fir_kernel
  D  Pipeline(2, 1): fe_mfma_kernel + resample_mfma_kernel (16-byte staging)
  E  fused mono bank, reference blocks, two calls: mono_fused_kernel over the pseudo-stream, channels_finish_kernel
  F  fused mono bank, smallest block, 65 535 .. 70 000 receivers: channels_finish_kernel's grid (nothing crosses 2^32)
  G  fast stereo bank   H  exact stereo bank   I  fast mono bank, mode 2: the slots cross

Pipelines: the input is a 1 MB FM stream tiled K times plus a ragged tail.  A control call of 3 periods + tail on the same
handle type is checked against the models exactly as the tests of that path do (bit for bit), and shown to be periodic;
the large call's periods 0 and 1 must equal the control's, every later period must equal period 1, the tail its prefix;
a second, small call on the same handle must continue the pattern (history, prev sample and discriminator tail taken
from the end of a block that ends past 2^32).  Banks: channel c carries stream c mod 16; a 32-channel control bank is
checked against the oracle / models, and channel c of the large bank must equal channel c mod 16.

Every output buffer is filled with a sentinel before a large call.  Each case prints its wall time and peak device
memory; it skips only if the device has less free memory than it needs."""
import math
import time

import numpy as np
import pytest

import _fe_model as fe
import _fir_model as fm
import _large_calls as lc
from test_gpu_channels import channel_stream
from test_gpu_fir_exact import bank_streams, concat, offsets, taps_of
from test_gpu_mfma_exact import check_fused, run_fused
from test_gpu_parity import assert_audio_close, assert_pcm_close

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CROSS = max(lc.BOUNDARIES) + lc.MARGIN
MAX_BANK = 70000        # receivers of the largest bank below


class Watch:
    """Free device memory before the case (skip below need + 2 GiB), the lowest seen since, wall time."""

    def __init__(self, case, need):
        import torch
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < need + 2 * GIB:
            pytest.skip(f"case {case}: {free} bytes of device memory free, the case needs {need} + 2 GiB")
        self.case, self.free0, self.low, self.t0, self.need = case, free, free, time.perf_counter(), need

    def sample(self):
        import torch
        self.low = min(self.low, torch.cuda.mem_get_info()[0])

    def done(self, note=""):
        import torch
        torch.cuda.empty_cache()
        print(f"large call, case {self.case}: wall {time.perf_counter() - self.t0:.1f} s, peak device memory "
              f"{(self.free0 - self.low) / 1e9:.1f} GB (planned {self.need / 1e9:.1f} GB){note}")


def same(got, want, msg):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, got.dtype)      # (the oracle's float32 values may arrive in a wider type)
    d, _ = lc._describe(got, want)
    assert not d, f"{msg}: {d}"


def sentinel(shape, f32):
    import torch
    if f32:
        return torch.full(shape, lc.F32_SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, lc.S16_SENTINEL, dtype=torch.int16, device="cuda")


# ---- pipelines (A - D) ------------------------------------------------------------------------------------------------
class Shape:
    """P, tails, K and the element counts of one pipeline case; asserts the rules of tests/_large_calls.py."""

    def __init__(self, p, periods, t1, t2, scale=(1, 1)):
        D, DA, U = p.rf_decim, p.audio_decim, p.audio_upsamp
        if U:                                   # the matrix-core resampler works on 16 output periods (DA IF samples each)
            self.unit, self.legal, self.sixteen = 2 * D * DA * 16, 2 * D * DA, 2 * D * DA * 16
            self.batch = self.unit
            self.in_per_audio = None
            self.audio_of = lambda nb: nb // (2 * D * DA) * U
        else:                                   # fused mono and the f32 matrix-core audio FIR: 256 audio outputs
            self.unit, self.legal, self.sixteen = 2 * D * DA * 256, math.lcm(2 * D * DA, 16), 2 * D * DA * 16
            self.batch = self.unit
            self.in_per_audio = 2 * D * DA
            self.audio_of = lambda nb: nb // (2 * D * DA)
        self.P, self.t1, self.t2 = periods * self.unit, t1 * self.legal, t2 * self.legal
        assert 1_000_000 <= self.P <= 1_100_000
        self.K = lc.periods_needed(self.P, self.unit, scale=scale)
        lc.check_tail(self.t1, self.P, self.legal, self.batch, self.sixteen)
        lc.check_tail(self.t2, self.P, self.legal, self.batch, self.sixteen)
        assert self.t1 != self.t2 and self.t1 % 16 == 0 and self.t2 % 16 == 0
        self.n1, self.n2 = self.K * self.P + self.t1, self.P + self.t2
        self.c1 = 3 * self.P + self.t1          # the control's first call
        self.if_of = lambda nb: nb // (2 * D)

    def streams(self, oracle, c, rf_Fs):
        """-> (base, the control's two blocks): the control's stream is the large one's with 3 periods for K."""
        base = channel_stream(oracle, c, self.P // 2, rf_Fs)
        lc.assert_no_alias("input", base)
        s = np.tile(base, 5)[:self.c1 + self.n2]
        return base, [s[:self.c1], s[self.c1:]]

    def control(self, name, a1, a2, of, bound=None):
        """The control's outputs of both calls are periodic: period 2 = period 1, tail = its prefix, the second call
        continues the pattern; and a wrapped offset cannot alias.  -> (period 0, period 1).  bound: the fused kernel's
        sums depend on an output's index IN ITS CALL mod 16 (tests/_fir_model.py: fused_audio) and the second call starts
        where the tail ended, not on a multiple of 16: there its outputs continue the pattern to within `bound` (f32) or
        1 LSB (s16) -- their bits are the model's (check_fused), and the large handle's must be the control's."""
        per, e1, e2 = of(self.P), of(self.t1), of(self.t2)
        assert len(a1) == 3 * per + e1 and len(a2) == per + e2, (name, len(a1), len(a2), per, e1, e2)
        p0, p1 = a1[:per], a1[per:2 * per]
        same(a1[2 * per:3 * per], p1, f"control, {name}: period 2 against period 1")
        same(a1[3 * per:], p1[:e1], f"control, {name}: tail against the start of period 1")
        want2 = lc.pattern(p1, e1, per + e2)
        if bound is None:
            same(a2, want2, f"control, {name}: second call against the pattern")
        else:
            d = np.abs(a2.astype(np.float64) - want2.astype(np.float64))
            if a2.dtype == np.int16:
                d = np.minimum(d, 65536 - d)
            worst = float(d.max())
            print(f"control, {name}: second call against the pattern, largest difference {worst:.3e} (bound {bound:.3e})")
            assert worst <= bound, (name, worst, bound)
        assert lc._describe(p0, p1)[0], f"control, {name}: period 0 equals period 1 (the stream's start is not silence?)"
        lc.assert_no_alias(name, p1)
        return p0, p1


def large_call(pl, d_iq, off, n_bytes, f32, pcm, wrap=True):
    import torch
    na = pl.n_audio(n_bytes)
    d_audio = sentinel((na,), True) if f32 else None
    d_pcm = sentinel((na,), False) if pcm else None
    torch.cuda.synchronize()
    pl.process_dev(d_iq.data_ptr() + off, n_bytes, d_audio.data_ptr() if f32 else None, d_pcm.data_ptr() if pcm else None, wrap=wrap)
    torch.cuda.synchronize()
    return d_audio, d_pcm


def run_plain(fmrx, mode, blocks, setup, taps=()):
    """The control of the unfused paths: audio, PCM and the taps of every block."""
    pl = fmrx.Pipeline(mode, 1, max_block_bytes=max(len(b) for b in blocks))
    setup(pl)
    out = []
    for blk in blocks:
        o = pl.process(blk)
        r = dict(audio=o["audio"], pcm=o["pcm16"], demod=pl.read_tap("demod"))
        r.update({t: pl.read_tap(t) for t in taps})
        out.append(r)
    pl.close()
    return out


def check_model(oracle, res, y_of, tag):
    """audio of every control block = the model's (bit for bit), PCM = the oracle's pack of it."""
    x = concat(res, "demod")
    for b, (lo, hi) in enumerate(offsets(res, "audio")):
        y = y_of(x, lo, hi - lo)
        same(res[b]["audio"], y, f"{tag}: control block {b}, audio against the model")
        np.testing.assert_array_equal(res[b]["pcm"], oracle.pcm16(y), f"{tag}: control block {b}, PCM")


def large_pipeline(fmrx, sh, tag, base, mode, setup, ctrl, res, watch, taps=(), tap_of=None):
    """One large call (f32 + PCM) and the small call behind it on one handle, against the control's periods."""
    import torch
    d_iq = torch.from_numpy(base).cuda().repeat(sh.K + 2)
    pl = fmrx.Pipeline(mode, 1, max_block_bytes=sh.n1)
    setup(pl)
    watch.sample()
    a, s = large_call(pl, d_iq, 0, sh.n1, True, True)
    watch.sample()
    per = sh.audio_of(sh.P)
    lc.check_periodic(f"{tag}: audio", a, per, sh.K, *ctrl["audio"], sh.in_per_audio)
    lc.check_periodic(f"{tag}: pcm", s, per, sh.K, *ctrl["pcm"], sh.in_per_audio)
    del a, s
    for t in taps:                              # the handle's own buffers: read back whole, compared on the host
        got = pl.read_tap(t)
        lc.check_periodic(f"{tag}: tap {t}", got, tap_of(sh.P), sh.K, *ctrl[t])
        del got
    a, s = large_call(pl, d_iq, sh.n1, sh.n2, True, True)
    same(a.cpu().numpy(), res[1]["audio"], f"{tag}: the call behind the large one, audio")
    same(s.cpu().numpy(), res[1]["pcm"], f"{tag}: the call behind the large one, pcm")
    for t in taps:
        same(pl.read_tap(t), res[1][t], f"{tag}: the call behind the large one, tap {t}")
    pl.close()
    del d_iq, a, s


def test_a_fused_mono_pipeline(fmrx, oracle):
    """Case A: the input (4.36 GB) crosses.  Control: run_fused / check_fused (tests/test_gpu_mfma_exact.py)."""
    import torch
    mode = 0
    p = fmrx.modeParams(mode)
    T, TA, D, DA = p.rf_taps, p.audio_taps, p.rf_decim, p.audio_decim
    sh = Shape(p, 41, 1237, 771)
    watch = Watch("A", int(3.3 * sh.n1))
    base, blocks = sh.streams(oracle, 4, p.rf_Fs)
    res = run_fused(fmrx, mode, T, TA, blocks)
    check_fused(oracle, res, taps_of(fmrx, p)[2], T, D, TA, DA, "case A, control", True)
    # two fmaf chains over the same TA products in another order differ by at most twice gamma sum |h x| (fm.gamma)
    h_au = taps_of(fmrx, p)[2]
    bound = 2 * fm.gamma(TA + 1) * float(np.abs(h_au).sum()) * float(max(np.abs(r["demod"]).max() for r in res))
    ctrl = {k: sh.control(k, res[0][k], res[1][k], sh.audio_of, bound if k == "audio" else 1)
            for k in ("audio", "pcm", "pcm_only_True", "pcm_only_False")}
    d_iq = torch.from_numpy(base).cuda().repeat(sh.K + 2)
    pl = fmrx.Pipeline(mode, 1, max_block_bytes=sh.n1)
    pl.set_option("fused_min_audio", 0)         # (the small call behind the large one takes the fused kernel too, as the control's)
    per = sh.audio_of(sh.P)
    for label, f32, wrap, key in (("f32 + PCM", True, True, "pcm"), ("PCM only, wrap", False, True, "pcm_only_True"),
                                  ("PCM only, saturate", False, False, "pcm_only_False")):
        pl.reset()
        a, s = large_call(pl, d_iq, 0, sh.n1, f32, True, wrap)
        watch.sample()
        if f32:
            lc.check_periodic(f"case A, {label}: audio", a, per, sh.K, *ctrl["audio"], sh.in_per_audio)
        lc.check_periodic(f"case A, {label}: pcm", s, per, sh.K, *ctrl[key], sh.in_per_audio)
        a, s = large_call(pl, d_iq, sh.n1, sh.n2, f32, True, wrap)
        if f32:
            same(a.cpu().numpy(), res[1]["audio"], f"case A, {label}: the call behind the large one, audio")
        same(s.cpu().numpy(), res[1][key], f"case A, {label}: the call behind the large one, pcm")
        del a, s
    pl.close()
    del d_iq
    watch.done()


def test_c_vector_alu_front_end(fmrx, oracle):
    """Case C: fe_demod_kernel (fe_variant valu) + audio_fir_kernel; the input crosses.  Control: audio = the polyphase
    fma chain of the demod tap bit for bit (tests/test_gpu_fir_exact.py), and within the mono tolerance of the oracle."""
    mode = 0
    p = fmrx.modeParams(mode)
    sh = Shape(p, 41, 1237, 771)
    watch = Watch("C", int(3.3 * sh.n1))
    base, blocks = sh.streams(oracle, 5, p.rf_Fs)
    setup = lambda pl: pl.set_option("fe_variant", "valu")
    res = run_plain(fmrx, mode, blocks, setup)
    h_au = taps_of(fmrx, p)[2]
    order = fm.polyphase(p.audio_taps, p.audio_decim)
    check_model(oracle, res, lambda x, lo, n: fm.fma_chain(x, h_au, order, p.audio_decim, 0, lo, n), "case C")
    ref = oracle.pipeline(mode, 1)
    for b, blk in enumerate(blocks):
        want = ref.process(blk)["audio"]
        assert_audio_close(res[b]["audio"], want, f"case C: control block {b} against the oracle")
        assert_pcm_close(res[b]["pcm"], oracle.pcm16(want))
    ctrl = {k: sh.control(k, res[0][k], res[1][k], sh.audio_of) for k in ("audio", "pcm")}
    large_pipeline(fmrx, sh, "case C", base, mode, setup, ctrl, res, watch)
    watch.done()


def test_d_matrix_core_resampler(fmrx, oracle):
    """Case D: mode 2, fe_mfma_kernel + resample_mfma_kernel; the input crosses.  Control: tests/test_gpu_mfma_exact.py's
    check of the resampler (the model fed the demod tap, bit for bit)."""
    mode = 2
    p = fmrx.modeParams(mode)
    sh = Shape(p, 4, 7, 11)
    watch = Watch("D", int(3.3 * sh.n1))
    base, blocks = sh.streams(oracle, 8, p.rf_Fs)
    res = run_plain(fmrx, mode, blocks, lambda pl: None)
    h_au = taps_of(fmrx, p)[2]
    check_model(oracle, res, lambda x, lo, n: fm.resample_mfma(x, h_au, p.audio_upsamp, p.audio_decim, 0, lo, n), "case D")
    exact = run_plain(fmrx, mode, blocks[:1], lambda pl: pl.set_option("resample_exact", 1))
    assert lc._describe(res[0]["audio"], exact[0]["audio"])[0], "case D: the control equals the resample_exact twin"
    ctrl = {k: sh.control(k, res[0][k], res[1][k], sh.audio_of) for k in ("audio", "pcm")}
    large_pipeline(fmrx, sh, "case D", base, mode, lambda pl: None, ctrl, res, watch)
    watch.done()


def test_b_kept_intermediates(fmrx, oracle):
    """Case B: mode 1 with the intermediates kept; the input (5.45 GB) and the interleaved IF buffer (0.8 x the input)
    cross.  Control: the IF taps = the integer model (tests/_fe_model.py), the demod tap = the reciprocal model of them
    (tests/test_gpu_demod_exact.py), audio = the polyphase fma chain of the demod tap -- all bit for bit.  The taps of the
    large call are the handle's own buffers: they cannot be pre-filled and come back whole through read_tap (the
    slow part of this case: 13 GB over a pageable copy, compared on the host)."""
    from test_gpu_demod_exact import check_demod
    mode = 1
    p = fmrx.modeParams(mode)
    D = p.rf_decim
    assert D == 5
    sh = Shape(p, 68, 1237, 771, scale=(4, 5))
    assert sh.if_of(sh.K * sh.P) * 8 >= CROSS
    watch = Watch("B", int(3.8 * sh.n1))
    base, blocks = sh.streams(oracle, 6, p.rf_Fs)
    taps = ("if_i", "if_q", "demod")

    def setup(pl):
        pl.set_keep_intermediates(True)

    res = run_plain(fmrx, mode, blocks, setup, taps=("if_i", "if_q"))
    h_rf = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, p.rf_taps)
    mi, mq = fe.fe_model(np.concatenate(blocks), np.full(2 * (p.rf_taps - 1), 128, np.uint8), h_rf, D)
    same(concat(res, "if_i"), mi, "case B: control, if_i against the integer model")
    same(concat(res, "if_q"), mq, "case B: control, if_q against the integer model")
    prev = (0.0, 0.0)
    for b, r in enumerate(res):
        check_demod(fmrx, r["demod"], r["if_i"], r["if_q"], prev, f"case B: control block {b}, demod")
        prev = (r["if_i"][-1], r["if_q"][-1])
    h_au = taps_of(fmrx, p)[2]
    order = fm.polyphase(p.audio_taps, p.audio_decim)
    check_model(oracle, res, lambda x, lo, n: fm.fma_chain(x, h_au, order, p.audio_decim, 0, lo, n), "case B")
    ctrl = {k: sh.control(k, res[0][k], res[1][k], sh.audio_of) for k in ("audio", "pcm")}
    ctrl.update({k: sh.control(k, res[0][k], res[1][k], sh.if_of) for k in taps})
    large_pipeline(fmrx, sh, "case B", base, mode, setup, ctrl, res, watch, taps=taps, tap_of=sh.if_of)
    watch.done("; read_tap of three 2.2 GB taps and their comparison on the host dominate")


# ---- banks (E - I) ----------------------------------------------------------------------------------------------------
def flat_rows(a):
    return np.ascontiguousarray(a).reshape(a.shape[0], -1)


def bank_control(fmrx, mode, kw, streams, calls, check):
    """A 32-channel bank, channel c on stream c mod 16: every call's audio / PCM rows [32, row]; `check(k, bank, out)` runs
    behind call k (taps); channels 16 - 31 equal channels 0 - 15.  -> (streams, pitch, block bytes, audio rows, pcm rows per call)"""
    ctl = fmrx.Channels(mode, 2 * lc.GROUP, **kw)
    bb = ctl.block_bytes
    assert len(streams) == lc.GROUP and all(len(st) == calls * bb for st in streams)
    pitch = ctl.input_layout()[1]
    audio, pcm = [], []
    for k in range(calls):
        out = ctl.process(np.stack([streams[c % lc.GROUP][k * bb:(k + 1) * bb] for c in range(2 * lc.GROUP)]))
        check(k, ctl, out)
        a, s = flat_rows(out["audio"]), flat_rows(out["pcm16"])
        same(a[lc.GROUP:], a[:lc.GROUP], f"control bank, call {k}: audio of channels 16 - 31 against 0 - 15")
        same(s[lc.GROUP:], s[:lc.GROUP], f"control bank, call {k}: pcm of channels 16 - 31 against 0 - 15")
        # (the outputs of the largest bank here end far below 2^31 bytes; their rule is kept for banks that grow)
        lc.assert_no_alias("bank audio", a[:lc.GROUP], total_bytes=MAX_BANK * a[0].nbytes)
        lc.assert_no_alias("bank pcm", s[:lc.GROUP], total_bytes=MAX_BANK * s[0].nbytes)
        slots = np.full((lc.GROUP, pitch), 128, np.uint8)
        slots[:, pitch - bb:] = np.stack([st[k * bb:(k + 1) * bb] for st in streams])
        lc.assert_no_alias("bank slots", slots)
        audio.append(a[:lc.GROUP].copy())
        pcm.append(s[:lc.GROUP].copy())
    ctl.close()
    return streams, pitch, bb, audio, pcm


def large_bank(fmrx, tag, mode, kw, N, streams, bb, pitch, audio, pcm, watch, reset_check=False):
    """N channels, channel c on stream c mod 16, one device call per control call: channel c against channel c mod 16 and the
    first 16 against the control bank's, f32 and PCM, on the device.  reset_check: then reset() (the whole bank's slots are
    filled with silence again) and the first call once more."""
    import torch
    ch = fmrx.Channels(mode, N, **kw)
    assert ch.input_layout()[1] == pitch and ch.block_bytes == bb
    q = -(-N // lc.GROUP)
    d_in = torch.empty((q * lc.GROUP, bb), dtype=torch.uint8, device="cuda")
    row_a, row_s = audio[0].shape[1], pcm[0].shape[1]

    def call(k, label):
        d16 = torch.from_numpy(np.stack([st[k * bb:(k + 1) * bb] for st in streams])).cuda()
        d_in.view(q, lc.GROUP, bb).copy_(d16.unsqueeze(0).expand(q, lc.GROUP, bb))
        d_audio, d_pcm = sentinel((N, row_a), True), sentinel((N, row_s), False)
        torch.cuda.synchronize()
        ch.load_dev(d_in.data_ptr())
        ch.process_dev(d_audio.data_ptr(), d_pcm.data_ptr())
        torch.cuda.synchronize()
        watch.sample()
        lc.check_channels(f"{tag}, {N} channels, {label}: audio", d_audio, audio[k], in_pitch=pitch)
        lc.check_channels(f"{tag}, {N} channels, {label}: pcm", d_pcm, pcm[k], in_pitch=pitch)

    for k in range(len(audio)):
        call(k, f"call {k}")
    if reset_check:
        ch.reset()
        call(0, "call 0 again after reset()")
    ch.close()
    del d_in
    torch.cuda.empty_cache()


def channels_past(pitch):
    """The smallest N with N pitch >= 2^32 + 64 MiB that leaves a ragged group of 5."""
    N = -(-CROSS // pitch)
    N += (5 - N) % lc.GROUP
    assert N <= MAX_BANK and N * pitch >= CROSS and N % lc.GROUP == 5
    return N


def oracle_mono_check(oracle, mode, streams, bb, tol_check):
    refs = [oracle.pipeline(mode, 1) for _ in streams]

    def check(k, bank, out):
        for c, st in enumerate(streams):
            want = refs[c].process(st[k * bb:(k + 1) * bb])["audio"]
            tol_check(out["audio"][c], out["pcm16"][c], want, f"control bank, channel {c}, call {k}")
    return check


def mono_tolerance(oracle, pcm_statistic=True):
    """The mono tolerance of tests/test_gpu_parity.py; its bound on the SHARE of s16 values one LSB off (1 %) needs blocks
    long enough to have a share: the 28-sample blocks of case F are held to the 1 LSB alone."""
    def tol(audio, pcm, want, msg):
        assert_audio_close(audio, want, msg)
        if pcm_statistic:
            assert_pcm_close(pcm, oracle.pcm16(want))
        else:
            d = np.abs(pcm.astype(np.int32) - oracle.pcm16(want).astype(np.int32))
            assert np.minimum(d, 65536 - d).max() <= 1, msg
    return tol


def test_e_fused_mono_bank(fmrx, oracle):
    """Case E: the fused mono bank at the reference block size, ~41 500 receivers: the slots (the fused kernel's
    pseudo-stream) cross.  Two calls: the second reads the history channels_finish_kernel moved at high addresses; then
    reset() and the first call again (every slot, also those past 2^32 bytes, holds silence again).
    Control: within the mono tolerance of the oracle per channel (tests/test_gpu_parity.py: test_many_channels_per_call)."""
    mode, kw, calls = 0, {}, 2
    p = fmrx.modeParams(mode)
    watch = Watch("E", int(2.4 * CROSS))
    bb = p.block_bytes
    pre = bank_streams(oracle, p, lc.GROUP, calls * bb // 2)
    streams, pitch, bb, audio, pcm = bank_control(fmrx, mode, kw, pre, calls, oracle_mono_check(oracle, mode, pre, bb, mono_tolerance(oracle)))
    N = channels_past(pitch)
    assert N * pitch >= CROSS and N % lc.GROUP
    large_bank(fmrx, "case E", mode, kw, N, streams, bb, pitch, audio, pcm, watch, reset_check=True)
    watch.done()


def smallest_bank_block(fmrx, mode):
    """The smallest block_bytes the fused mono bank accepts, found by asking it."""
    p = fmrx.modeParams(mode)
    unit = math.lcm(2 * p.rf_decim * p.audio_decim, 16)
    for k in range(1, 200):
        try:
            fmrx.Channels(mode, 1, block_bytes=k * unit).close()
            return k * unit
        except fmrx.FmrxError as e:
            assert e.code == fmrx.EINVAL
    raise AssertionError("no block of up to 200 units accepted")


@pytest.fixture(scope="module")
def grid_control(fmrx, oracle):
    mode = 0
    bb = smallest_bank_block(fmrx, mode)
    kw = dict(block_bytes=bb)
    p = fmrx.modeParams(mode)
    pre = bank_streams(oracle, p, lc.GROUP, 2 * bb // 2)
    return kw, bank_control(fmrx, mode, kw, pre, 2, oracle_mono_check(oracle, mode, pre, bb, mono_tolerance(oracle, False)))


@pytest.mark.parametrize("N", [65535, 65536, 65537, 70000])
def test_f_bank_grid(fmrx, oracle, grid_control, N):
    """Case F: the fused mono bank at its smallest block with more receivers than a grid's y holds (0.4 GB: nothing
    crosses).  channels_finish_kernel carries the channel in its grid's x, so every N is served: two calls right for
    every channel.  (A create that refused with FMRX_EINVAL and named the limit would be the other legal answer; an error
    from process, a wrong channel or a failure found at synchronisation is a bug.)"""
    kw, (streams, pitch, bb, audio, pcm) = grid_control
    watch = Watch(f"F, {N} channels", int(2.5 * N * pitch))
    try:
        fmrx.Channels(0, N, **kw).close()
    except fmrx.FmrxError as e:
        assert e.code == fmrx.EINVAL and "n_channels" in str(e) and any(ch.isdigit() for ch in str(e)), e
        pytest.fail(f"create refuses {N} channels although the README advertises 65 536 and more: {e}")
    large_bank(fmrx, "case F", 0, kw, N, streams, bb, pitch, audio, pcm, watch)
    watch.done()


def test_g_fast_stereo_bank(fmrx, oracle):
    """Case G: the fast stereo bank, one reference block, one call from reset; the slots cross.  Control: left / right
    against the fma-chain model of the bank's own taps (tests/test_gpu_fir_exact.py: test_fast_stereo_bank) and trigArg
    / NCO against the PLL model (tests/test_gpu_pll_exact.py: check_bank), bit for bit."""
    from test_gpu_pll_exact import check_bank
    mode, kw = 0, dict(audio_channels=2, exact=False)
    p = fmrx.modeParams(mode)
    watch = Watch("G", int(3.5 * CROSS))
    h_st, _, h_au = taps_of(fmrx, p)
    D, delay = p.audio_decim, (p.stereo_taps - 1) // 2

    def check(k, bank, out):
        t = {n: np.stack([bank.read_tap(c, n) for c in range(lc.GROUP)]) for n in ("demod", "carrier_filt", "stereo_filt", "pll", "trig_arg")}
        check_bank(fmrx, p, [t], "case G, control bank")
        for c in range(lc.GROUP):
            x, tag = t["demod"][c], f"case G, control bank, channel {c}"
            same(t["stereo_filt"][c], fm.fma_chain(x, h_st, fm.ascending(p.stereo_taps)), tag + ": stereo_filt")
            mono, st = fm.audio_pair(x, fm.mixer(t["stereo_filt"][c], t["pll"][c]), h_au, D, delay, fm.ascending(p.audio_taps))
            left, right = fm.combine(st, mono)
            same(out["audio_l"][c], left, tag + ": left")
            same(out["audio_r"][c], right, tag + ": right")
            np.testing.assert_array_equal(out["pcm16"][c, :, 0], oracle.pcm16(left), tag)
            np.testing.assert_array_equal(out["pcm16"][c, :, 1], oracle.pcm16(right), tag)

    streams, pitch, bb, audio, pcm = bank_control(fmrx, mode, kw, bank_streams(oracle, p, lc.GROUP, p.block_bytes // 2), 1, check)
    N = channels_past(pitch)
    large_bank(fmrx, "case G", mode, kw, N, streams, bb, pitch, audio, pcm, watch)
    watch.done()


def test_h_exact_stereo_bank(fmrx, oracle):
    """Case H: the exact stereo bank (chs_fe_exact_kernel, pll_channels_kernel, the exact output kernels), one call; the
    slots cross.  Control: left, right and PCM bit for bit against the oracle (tests/test_gpu_channels.py)."""
    mode, kw = 0, dict(audio_channels=2, exact=True)
    p = fmrx.modeParams(mode)
    watch = Watch("H", int(3.5 * CROSS))
    bb = p.block_bytes
    pre = bank_streams(oracle, p, lc.GROUP, bb // 2)

    def check(k, bank, out):
        for c, st in enumerate(pre):
            want = oracle.pipeline(mode, 2).process(st[:bb])
            tag = f"case H, control bank, channel {c}"
            same(bank.read_tap(c, "demod"), want["demod"], tag + ": demod")
            same(out["audio_l"][c], want["audio_l"], tag + ": left")
            same(out["audio_r"][c], want["audio_r"], tag + ": right")
            same(out["pcm16"][c, :, 0], oracle.pcm16(want["audio_l"]), tag + ": pcm left")
            same(out["pcm16"][c, :, 1], oracle.pcm16(want["audio_r"]), tag + ": pcm right")

    streams, pitch, bb, audio, pcm = bank_control(fmrx, mode, kw, pre, 1, check)
    N = channels_past(pitch)
    large_bank(fmrx, "case H", mode, kw, N, streams, bb, pitch, audio, pcm, watch)
    watch.done()


def test_i_fast_mono_bank_resampling(fmrx, oracle):
    """Case I: the fast mono bank of mode 2 (fe_mfma_bank_kernel, chs_resample_lanes_kernel), one call; the slots cross.
    Control: audio RMS error <= 2e-6 against the oracle, s16 within 1 LSB (tests/test_gpu_channels.py:
    test_bank_fast_resampling_modes)."""
    mode, kw = 2, {}
    p = fmrx.modeParams(mode)
    watch = Watch("I", int(3.0 * CROSS))
    bb = p.block_bytes
    pre = bank_streams(oracle, p, lc.GROUP, bb // 2)

    def tol(audio, pcm, want, msg):
        err = float(np.sqrt(np.mean((audio.astype(np.float64) - want) ** 2)))
        assert err <= 1e-4 and err <= 2e-6, (msg, err)
        assert np.abs(pcm.astype(np.int32) - oracle.pcm16(want).astype(np.int32)).max() <= 1, msg

    streams, pitch, bb, audio, pcm = bank_control(fmrx, mode, kw, pre, 1, oracle_mono_check(oracle, mode, pre, bb, tol))
    N = channels_past(pitch)
    large_bank(fmrx, "case I", mode, kw, N, streams, bb, pitch, audio, pcm, watch)
    watch.done()
