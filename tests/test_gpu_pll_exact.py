"""The PLL's FAST recurrence on the device checked against the float model of tests/_pll_model.py, and the serial glibc
form of the single-stream pipeline against the oracle's fmPLL.

  fast stereo bank, modes 0/1   the raw trigArg row (FMRX_TAP_TRIG_ARG) BIT FOR BIT against the model run from the reset
                                state over every call on the carrier sign row the bank's PLL reads (FMRX_TAP_CARRIER, itself
                                checked against the sign of the fma-chain model of the pilot band-pass output); the NCO tap
                                within NCO_EPS of cos(2 pi r_model)
  fast stereo bank, modes 2/3   the NCO tap within NCO_EPS of the model
  cut invariance                the same streams through fast banks of 1, 2, 4 and 8 reference blocks per call: trigArg (or
                                NCO) rows and L / R bit-identical -- the PLL is launched once per chunk and call, and the
                                fast bank carries the loop's angle fr itself across those seams (state slot 6)
  pipeline, pll_mode 2          serial, glibc's functions on the specialised upstream: NCO tap and the PLL's six state
                                floats equal oracle.fm_pll of the pipeline's own carrier_filt tap bit for bit
  pipeline, pll_mode 1          serial, fast math, a 1,024,000-sample first call: integ, phase, trigOffset equal the model
                                bit for bit, the NCO within NCO_EPS (later calls rebuild fr from the carried feedback pair
                                with the device's atan2f: left to tests/test_gpu_parity.py)

NCO_EPS (tests/_pll_model.py) bounds |v_cos_f32(r) - cos(2 pi r)| for r in [-0.5, 0.5] revolutions.  Measured by this file
on an MI355X as the largest difference over every compared sample: 1.25e-7 over 1.7e7 samples (the tests print it); the
bound is 5e-7, 4 x that.  One grid step of trigArg moves the NCO by >= 2 ulp(trigArg) |sin|, 7.8e-3 after 0.5 s of stream,
and a model with Ki one ulp off leaves NCO_EPS (asserted below).

Before the fast bank carried fr in state slot 6 (it rebuilt it at every launch as atan2f(fbQ, fbI) / 2 pi from the
hardware cos / sin of it), trigArg changed bits at seams: modes 0/1 with 8 blocks per call against 1 (whose chunk seams
differ), modes 2/3 already with 2 -- and the model tests failed on the first seam inside a lane's lock; the bank's audio
envelope test (test_gpu_channels.py::test_stereo_bank_fast_error_envelope) passed either way."""
import math

import numpy as np
import pytest

import _fir_model as fm
import _pll_model as pm
from test_gpu_channels import channel_stream
from test_gpu_fir_exact import bits_equal, block_cuts, feed, silence_then_full_scale, taps_of

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MEASURED = {"eps": 0.0, "n": 0}
ZERO_RUN_LANES = (1, 2)        # streams with runs of v = 0 (silence, drop-out): the only lanes that may meet an undetermined step


def nco_close(got, r_model, msg):
    """|device NCO - cos(2 pi r)| <= NCO_EPS, sample for sample; records the largest difference."""
    d = np.abs(np.asarray(got, F64) - np.cos(2 * math.pi * np.asarray(r_model, F64)))
    MEASURED["eps"] = max(MEASURED["eps"], float(d.max(initial=0.0)))
    MEASURED["n"] += d.size
    bad = np.flatnonzero(d > pm.NCO_EPS)
    assert len(bad) == 0, f"{msg}: {len(bad)} of {d.size} NCO values off by more than {pm.NCO_EPS}, first at {bad[0]}: {d[bad[0]]:.3e}"


def report():
    print(f"NCO: max |v_cos_f32(r) - cos(2 pi r)| so far {MEASURED['eps']:.3e} over {MEASURED['n']} samples")


def no_pilot_stream(n_samples, rf_Fs, seed=3):
    """Mono FM (a 1 kHz tone and noise, 75 kHz deviation) without the 19 kHz pilot, as u8 I/Q."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples) / rf_Fs
    msg = 0.8 * np.sin(2 * np.pi * 1e3 * t) + 0.1 * rng.standard_normal(n_samples)
    ph = 2 * np.pi * 75e3 / rf_Fs * np.cumsum(msg)
    iq = np.empty(2 * n_samples, np.uint8)
    iq[0::2] = np.clip(np.round(127.5 + 100 * np.cos(ph)), 0, 255)
    iq[1::2] = np.clip(np.round(127.5 + 100 * np.sin(ph)), 0, 255)
    return iq


def bank_inputs(oracle, p, N, n_samples):
    """Channel streams: synthetic (locked pilot) everywhere, channel 1 silence then full-scale bytes (the v = 0 path),
    channel 2 a locked stream with a run of zero bytes in the middle (a drop-out), channel 3 no pilot."""
    s = [channel_stream(oracle, c, n_samples, p.rf_Fs) for c in range(N)]
    s[1] = silence_then_full_scale(n_samples, n_samples // 3, seed=11)
    lo = 2 * (n_samples // 2)
    s[2][lo:lo + 2 * (n_samples // 20)] = 0
    s[3] = no_pilot_stream(n_samples, p.rf_Fs)
    return s


def run_bank(fmrx, mode, taps, N, bb, calls, streams, reset=None, raw=True):
    """Feed `calls` blocks of bb bytes per channel; after call reset[0] channel reset[1] is reset and starts its stream
    anew.  Returns per call: the taps of every channel, L and R."""
    ch = fmrx.Channels(mode, N, rf_taps=taps[0], base_audio_taps=taps[1], stereo_taps=taps[2], audio_channels=2, exact=False,
                       block_bytes=bb)
    pos = [0] * N
    out = []
    for k in range(calls):
        blk = np.stack([streams[c][pos[c]:pos[c] + bb] for c in range(N)])
        pos = [q + bb for q in pos]
        o = ch.process(blk, want_pcm=False)
        r = {"audio_l": o["audio_l"].copy(), "audio_r": o["audio_r"].copy()}
        for t in ("demod", "carrier_filt", "pll") + (("trig_arg",) if raw else ()):
            r[t] = np.stack([ch.read_tap(c, t) for c in range(N)])
        out.append(r)
        if reset and k == reset[0]:
            ch.reset(reset[1])
            pos[reset[1]] = 0
    if not raw:
        with pytest.raises(fmrx.FmrxError):
            ch.read_tap(0, "trig_arg")
    ch.close()
    return out


def model_bank(fmrx, p, calls, reset=None):
    """The carrier signs (checked against the sign of the fma-chain model of the pilot filter on the bank's own demod rows)
    and the model's trigArg per call, every lane from the reset state; a reset lane restarts at its reset."""
    _, h_car, _ = taps_of(fmrx, p)
    c = pm.coef(19e3, float(p.if_Fs))
    N = calls[0]["demod"].shape[0]
    edges = np.concatenate([[0], np.cumsum([blk["demod"].shape[1] for blk in calls])])
    sign = np.concatenate([blk["carrier_filt"] for blk in calls], axis=1)
    demod = np.concatenate([blk["demod"] for blk in calls], axis=1)
    segs = [(lane, 0, edges[-1]) for lane in range(N)]
    if reset:
        cut = edges[reset[0] + 1]
        segs[reset[1]] = (reset[1], 0, cut)
        segs.append((reset[1], cut, edges[-1]))
    for lane, lo, hi in segs:
        want = pm.carrier_sign(fm.fma_chain(demod[lane, lo:hi], h_car, fm.ascending(p.stereo_taps)))
        bits_equal(sign[lane, lo:hi], want, f"carrier sign, lane {lane} [{lo}, {hi})")
    trig, _, und = pm.run(sign, c)
    if reset:
        lane, cut = reset[1], edges[reset[0] + 1]
        t2, _, u2 = pm.run(sign[lane, cut:], c)
        trig[lane, cut:] = t2
        if und[lane] < 0 or und[lane] >= cut:
            und[lane] = -1 if u2 < 0 else cut + u2
    return c, trig, und, edges


def check_bank(fmrx, p, calls, tag, reset=None, raw=True):
    c, trig, und, edges = model_bank(fmrx, p, calls, reset)
    N = trig.shape[0]
    r = pm.nco_arg(trig, c)
    print(f"{tag}: undetermined (lane, step) {[(i, int(u)) for i, u in enumerate(und) if u >= 0]}")
    assert (und[[i for i in range(N) if i not in ZERO_RUN_LANES]] < 0).all()
    for k, blk in enumerate(calls):
        lo, hi = edges[k], edges[k + 1]
        for lane in range(N):
            stop = hi if und[lane] < 0 else min(hi, und[lane])
            if stop <= lo:
                continue
            msg = f"{tag}: call {k}, channel {lane}"
            if raw:
                bits_equal(blk["trig_arg"][lane, :stop - lo], trig[lane, lo:stop], msg + ", trigArg")
            nco = blk["pll"][lane]
            nco_close(nco[1:stop - lo + 1], r[lane, lo:stop], msg + ", NCO")
            if k == 0 or (reset and k == reset[0] + 1 and lane == reset[1]):
                assert nco[0] == 1.0, msg
            else:
                nco_close(nco[:1], r[lane, lo - 1:lo], msg + ", PLL[0]")
    report()
    return c, trig


# (mode, taps, receivers, reference blocks per call, calls): 24 receivers (one wave) and 65 (two, the second with one lane)
BANK_CASES = [(0, (101, 101, 101), 24, 1, 5), (0, (101, 101, 101), 65, 4, 5), (1, (101, 101, 101), 24, 4, 3),
              (1, (13, 13, 13), 65, 1, 5), (0, (151, 101, 151), 24, 4, 5)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_fast_bank_cut_invariance(fmrx, oracle, mode):
    """Five receivers, eight reference blocks of stream, through fast banks of 1, 2, 4 and 8 blocks per call (the PLL is
    launched once per chunk: 2 .. 8 chunks per call): the raw trigArg rows (modes 0/1; modes 2/3: the NCO rows) and left /
    right are bit-identical whatever the cut."""
    p = fmrx.modeParams(mode)
    N, nblk = 5, 8
    streams = bank_inputs(oracle, p, N, nblk * p.block_bytes // 2)
    raw = mode < 2
    got = {}
    for per in (1, 2, 4, 8):
        calls = run_bank(fmrx, mode, (101, 101, 101), N, per * p.block_bytes, nblk // per, streams, raw=raw)
        got[per] = {t: np.concatenate([blk[t] for blk in calls], axis=1) for t in ("audio_l", "audio_r")}
        got[per]["row"] = np.concatenate([blk["trig_arg"] if raw else blk["pll"][:, 1:] for blk in calls], axis=1)
    for per in (2, 4, 8):
        for t in ("row", "audio_l", "audio_r"):
            for c in range(N):
                bits_equal(got[per][t][c], got[1][t][c], f"mode {mode}: {t}, channel {c}, {per} blocks per call vs 1")


@pytest.mark.parametrize("mode,taps,N,per_call,calls", BANK_CASES)
def test_fast_bank_trig_arg_is_the_model(fmrx, oracle, mode, taps, N, per_call, calls):
    """Fast bank, modes 0/1: trigArg bit for bit, NCO within NCO_EPS, over every call from the reset state.  Channels: locked
    synthetic streams, silence then full scale (channel 1: the zero-sample path), a drop-out (2), no pilot (3), and channel
    N - 2 reset after the second call (a new stream there while the others carry on)."""
    p = fmrx.modeParams(mode, *taps)
    bb = per_call * p.block_bytes
    streams = bank_inputs(oracle, p, N, calls * bb // 2)
    reset = (1, N - 2)
    out = run_bank(fmrx, mode, taps, N, bb, calls, streams, reset=reset)
    c, _ = check_bank(fmrx, p, out, f"fast bank mode {mode} taps {taps} N {N} x {per_call}", reset=reset)
    if N == 65 and per_call == 4:
        # a loop constant one ulp off: the model leaves the device's NCO by more than NCO_EPS (the bound tells them apart)
        sign = np.concatenate([blk["carrier_filt"][0] for blk in out])
        moved, _, _ = pm.run(sign, pm.Coef(c.Kp, np.nextafter(c.Ki, F32(1)), c.w, c.nco_scale, c.phase_adjust))
        nco = np.concatenate([blk["pll"][0, 1:] for blk in out])
        assert (np.abs(nco - np.cos(2 * math.pi * pm.nco_arg(moved, c).astype(F64))) > pm.NCO_EPS).any()


@pytest.mark.parametrize("mode", [2, 3])
def test_fast_bank_resampling_modes_nco_is_the_model(fmrx, oracle, mode):
    """Fast bank, modes 2/3 (the NCO pass overwrites trigArg in place; FMRX_TAP_TRIG_ARG refuses): the NCO tap within
    NCO_EPS of the model, the same kinds of stream, a reset mid-stream."""
    p = fmrx.modeParams(mode)
    N, calls = 24, 5
    streams = bank_inputs(oracle, p, N, calls * p.block_bytes // 2)
    reset = (1, N - 2)
    out = run_bank(fmrx, mode, (101, 101, 101), N, p.block_bytes, calls, streams, reset=reset, raw=False)
    check_bank(fmrx, p, out, f"fast bank mode {mode}", reset=reset, raw=False)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pipeline_serial_glibc_pll_is_the_oracle(fmrx, oracle, mode):
    """pll_mode 2 (serial, glibc's functions) on the specialised upstream: the NCO tap and the PLL's six state floats equal
    oracle.fm_pll run on the pipeline's own carrier_filt tap bit for bit, over ragged blocks."""
    p = fmrx.modeParams(mode)
    cuts = block_cuts(p, True)
    iq = channel_stream(oracle, 5, sum(cuts) * p.rf_decim, p.rf_Fs)
    pl = fmrx.Pipeline(mode, 2, max_block_bytes=2 * max(cuts) * p.rf_decim)
    pl.set_option("pll_mode", 2)
    st = np.array([0, 0, 1, 0, 1, 0], F32)
    for k, blk in enumerate(feed(cuts, p, iq)):
        pl.process(blk, want_pcm=False)
        car = pl.read_tap("carrier_filt")
        want, st = oracle.fm_pll(car, st, 19e3, float(p.if_Fs))
        bits_equal(pl.read_tap("pll"), want, f"mode {mode}, block {k}: NCO")
        bits_equal(pl.get_state()[-6:], st, f"mode {mode}, block {k}: PLL state")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pipeline_serial_fast_pll_is_the_model(fmrx, oracle, mode):
    """pll_mode 1 (serial, fast math), a stream's first call of ~1,024,000 complex samples: integ, phase and trigOffset of
    get_state() equal the model bit for bit; the NCO is within NCO_EPS for every sample."""
    p = fmrx.modeParams(mode)
    nblk = max(1, round(1_024_000 / (p.block_bytes // 2)))
    iq = channel_stream(oracle, 0, nblk * p.block_bytes // 2, p.rf_Fs)
    pl = fmrx.Pipeline(mode, 2, max_block_bytes=len(iq))
    pl.set_option("pll_mode", 1)
    pl.process(iq, want_pcm=False)
    car = pl.read_tap("carrier_filt")
    c = pm.coef(19e3, float(p.if_Fs))
    trig, st, und = pm.run(car, c)
    assert und == -1
    nco = pl.read_tap("pll")
    assert nco[0] == 1.0
    nco_close(nco[1:], pm.nco_arg(trig, c), f"mode {mode}: NCO")
    s = pl.get_state()[-6:]
    bits_equal(s[[0, 1, 5]], np.array([st.integ[0], st.phase[0], st.off[0]], F32), f"mode {mode}: integ, phase, trigOffset")
    report()
