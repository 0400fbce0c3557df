"""The two fast MONO banks checked BIT FOR BIT against the fma-chain models of tests/_fir_model.py: no tolerance anywhere,
float outputs compared as uint32, PCM as integers.

  the fused mono bank of modes 0/1 (bank.hip: mono_fused_kernel over all slots as one pseudo-stream, then
  channels_finish_kernel) = fused_audio(row0 = the row of the channel's first kept output in the launch), fed the
  discriminator stream of a twin single-stream pipeline that saw this channel's samples alone, in the same cuts.  A
  neighbour's sample in a window, a wrong history byte at the seam between calls, a junk count off by one, a wrong
  destination row in the finish kernel, a reset that touches another channel: each changes bits.  The geometry is read
  from the handle (input_layout): hist = pitch - block_bytes, junk = hist / unit, slot_audio = pitch / unit, row phase of
  channel c = (c slot_audio + junk) mod 16.

  the fast mono bank of modes 2/3 (kernels_bank.hip: chs_resample_lanes_kernel<STEREO = false>, two outputs per packed
  instruction, 7 waves per workgroup) = resample_chain over the bank's own demod tap, which for a subset of channels
  equals the single-stream pipeline's bit for bit.

Where the row phase changes bits: fm.row_phase_changes_bits (every phase but 0 at DA = 5; 4 and 12 at DA = 6, where phase 8
moves every tap by three whole MFMA groups and leaves the bits of phase 0).  Channels on the synthetic stream with >= 1000
outputs per call must differ from the two-kernel path's polyphase chain, and from the row0 = 0 model wherever the phase
changes bits: the test would notice a model that ignores the phase.

launch_resample's rule for the groups of 7 outputs a wave walks (kernels_bank.hip), restated by groups_per_wave():
    gpw = U / 7;  while gpw > NW and ceil(N / 64) periods ceil((U / 7) / gpw) NW < 8192: gpw = ceil(gpw / 2);
    gpw = NW ceil(gpw / NW);  NW = 7 (mono), 3 (stereo);  a wave walks gpw / NW groups
`periods` is what one launch covers: the whole call of a mono bank, one chunk (ceil(periods per call / 8)) of a stereo
bank.  X = ceil(N / 64) periods: mono mode 3 walks 2 groups from X = 147, 3 from X = 293; stereo mode 3 walks 2 from X = 171.
The multi-group tests derive their receiver counts from these and assert what the rule gives.

Every test prints the row phases it met, or X and the groups per wave."""
import math

import numpy as np
import pytest

import _fir_model as fm
from test_gpu_channels import channel_stream
from test_gpu_demod_exact import weak_bytes
from test_gpu_fir_exact import MIN_POWER, bits, bits_equal, differs, silence_then_full_scale, taps_of
from test_gpu_mfma_exact import FUSED_CASES, MODE_OF_DECIM

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT16, SENT32 = 0x5A5A, 0x7FC5A5A5          # sentinels of the device-side output buffers (the f32 one a NaN)
RECEIVERS = [1, 7, 70]
BLOCK_KINDS = ["reference", "smallest", "ragged", "phases"]
FULL_SHAPES = [(101, 10, 101, 5), (101, 5, 101, 6)]
FUSED_BANK_CASES = ([s + (n, k) for s in FULL_SHAPES for n in RECEIVERS for k in BLOCK_KINDS]
                    + [s + (7, k) for s in FUSED_CASES if s not in FULL_SHAPES for k in ("smallest", "phases")])
# block 0, 1, 2; one middle channel starts a new stream; blocks 3, 4; every channel starts again; block 0
STEPS = [("call", 0), ("call", 1), ("call", 2), ("reset", "middle"), ("call", 3), ("call", 4), ("reset", -1), ("call", 0)]
N_BLOCKS = 5

_streams = {}


def cached_stream(oracle, c, n_samples, rf_Fs):
    """Channel c's synthetic stream, generated once at the longest length asked for (any prefix is as good a stream)."""
    key = (c, float(rf_Fs))
    if key not in _streams or len(_streams[key]) < 2 * n_samples:
        _streams[key] = channel_stream(oracle, c, n_samples, rf_Fs)
    return _streams[key][:2 * n_samples]


def fused_streams(oracle, p, N, n_samples, salt=0):
    """Distinct streams; channel 1 silence then full scale; channel 2 weak (sparse 127 / 129 bytes in silence) between it and
    channel 3 of random 0 / 255 bytes: leakage from either neighbour would be large against channel 2's own signal."""
    s = [cached_stream(oracle, c + 100 * salt, n_samples, p.rf_Fs) for c in range(N)]
    kinds = ["synthetic"] * N
    if N > 1:
        s[1], kinds[1] = silence_then_full_scale(n_samples, n_samples // 3, seed=11 + salt), "silence"
    if N > 3:
        rng = np.random.default_rng(21 + salt)
        s[2], kinds[2] = weak_bytes(rng, 2 * n_samples), "weak"
        s[3], kinds[3] = rng.integers(0, 2, 2 * n_samples).astype(np.uint8) * 255, "full scale"
    return s, kinds


def bank_of(fmrx, mode, T, TA, N, bb):
    return fmrx.Channels(mode, N, rf_taps=T, base_audio_taps=TA, block_bytes=bb)


def smallest_fused_block(fmrx, mode, T, TA):
    """The smallest block_bytes the fused mono bank accepts at these taps, found by asking it."""
    p = fmrx.modeParams(mode, T, TA)
    unit = math.lcm(2 * p.rf_decim * p.audio_decim, 16)
    for k in range(1, 200):
        try:
            bank_of(fmrx, mode, T, TA, 1, k * unit).close()
            return k * unit
        except fmrx.FmrxError as e:
            assert e.code == fmrx.EINVAL
    raise AssertionError("no block of up to 200 units accepted")


def geometry(ch, p):
    """(junk outputs in front of a slot, outputs per slot, row phase of every channel's first kept output), from the handle."""
    _, pitch = ch.input_layout()
    unit = 2 * p.rf_decim * p.audio_decim
    hist = pitch - ch.block_bytes
    assert hist > 0 and hist % unit == 0 and pitch % unit == 0
    junk, slot_audio = hist // unit, pitch // unit
    return junk, slot_audio, [(c * slot_audio + junk) % 16 for c in range(ch.n_channels)]


def block_bytes_of(fmrx, mode, T, TA, kind):
    p = fmrx.modeParams(mode, T, TA)
    unit = 2 * p.rf_decim * p.audio_decim
    small = smallest_fused_block(fmrx, mode, T, TA)
    if kind == "reference":
        return p.block_bytes
    if kind == "smallest":
        return small
    if kind == "ragged":
        return (256 * 5 + 100) * unit                # several batches of the kernel and a ragged rest
    # "phases": slots 4 (mod 16) outputs long, so that four consecutive channels meet the phases 0, 4, 8, 12
    ch = bank_of(fmrx, mode, T, TA, 1, small)
    junk = geometry(ch, p)[0]
    ch.close()
    n = next(n for n in range(MIN_POWER, MIN_POWER + 64, 4) if (junk + n) % 16 == 4)
    return n * unit


def device_outputs(torch, N, na, want_f32, want_pcm, skew=0):
    """Sentinel-filled device buffers one row longer than the call needs; skew: elements past 16-byte alignment."""
    f = torch.full(((N + 1) * na + 8,), SENT32, dtype=torch.int32, device="cuda") if want_f32 else None
    s = torch.full(((N + 1) * na + 8,), SENT16, dtype=torch.int16, device="cuda") if want_pcm else None
    for t in (f, s):
        assert t is None or t.data_ptr() % 16 == 0
    return f, s, (f.data_ptr() + 4 * skew if want_f32 else None), (s.data_ptr() + 2 * skew if want_pcm else None)


def read_outputs(f, s, N, na, skew, msg):
    """-> (audio [N, na] or None, pcm [N, na] or None); everything around the N rows still holds the sentinel."""
    out = []
    for t, sent in ((f, SENT32), (s, SENT16)):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[:skew] == sent).all() and (a[skew + N * na:] == sent).all(), msg + ": written outside the N rows"
        body = a[skew:skew + N * na].reshape(N, na)
        out.append(body.view(F32) if sent == SENT32 else body)
    return out


VARIANTS = {"pcm_wrap": (False, True, True, 0), "pcm_saturate": (False, True, False, 0), "f32_only": (True, False, True, 0),
            "unaligned": (True, True, True, 1)}      # (f32, PCM, wrap, skew)


def drive_fused(fmrx, mode, T, TA, N, bb, streams, middle, variants=()):
    """One handle through STEPS by process() ("host": f32 + PCM) and one per variant by load_dev / process_dev.
    -> {name: [per call (audio, pcm)]}, geometry."""
    import torch
    p = fmrx.modeParams(mode, T, TA)
    banks = {k: bank_of(fmrx, mode, T, TA, N, bb) for k in ("host",) + tuple(variants)}
    geo = geometry(banks["host"], p)
    na = banks["host"].n_audio
    assert na == bb // (2 * p.rf_decim * p.audio_decim)
    res = {k: [] for k in banks}
    for op, arg in STEPS:
        if op == "reset":
            for b in banks.values():
                b.reset(middle if arg == "middle" else arg)
            continue
        iq = np.stack([s[arg * bb:(arg + 1) * bb] for s in streams])
        o = banks["host"].process(iq)
        res["host"].append((o["audio"], o["pcm16"]))
        d_iq = torch.from_numpy(iq).cuda()
        for k in variants:
            want_f32, want_pcm, wrap, skew = VARIANTS[k]
            f, s, pf, ps = device_outputs(torch, N, na, want_f32, want_pcm, skew)
            banks[k].load_dev(d_iq.data_ptr())
            banks[k].process_dev(pf, ps, wrap=wrap)
            torch.cuda.synchronize()
            res[k].append(read_outputs(f, s, N, na, skew, f"{k}, call {len(res[k])}"))
    for b in banks.values():
        b.close()
    return res, geo


def twin_streams(fmrx, mode, T, TA, bb, stream, c, middle):
    """The discriminator stream of a single-stream pipeline (two-kernel path, intermediates kept: the tap pinned by
    tests/test_gpu_demod_exact.py) fed channel c's blocks alone, in the bank's cuts.  -> per call (stream since its start,
    index of the call's first output in it, in calls)."""
    def make():
        pl = fmrx.Pipeline(mode, 1, rf_taps=T, base_audio_taps=TA, max_block_bytes=bb)
        pl.set_option("fused_min_audio", 10 ** 12)
        pl.set_keep_intermediates(True)
        return pl
    pl, xs, out = make(), [], []
    for op, arg in STEPS:
        if op == "reset":
            if arg == -1 or c == middle:
                pl.close()
                pl, xs = make(), []
            continue
        pl.process(stream[arg * bb:(arg + 1) * bb], want_pcm=False)
        xs.append(pl.read_tap("demod"))
        out.append((np.concatenate(xs), len(xs) - 1))
    pl.close()
    return out


def batch(segs, n, TA, DA):
    """Segments (stream, first output k0), n outputs each, laid one behind the other for ONE run of a model: each keeps the
    samples its outputs reach (zeros in front of the stream's start) behind a multiple of 16 outputs of zeros, so that
    output j of segment i sits at index i * pitch + front + j, and at row (row0 + j) mod 16 of fused_audio(row0)."""
    front = 16 * -(-(TA + 16 * DA) // (16 * DA))
    pitch = front + 16 * -(-n // 16)
    cat = np.zeros(len(segs) * pitch * DA, F32)
    for i, (x, k0) in enumerate(segs):
        lo = max(0, DA * k0 - DA * front)
        at = (i * pitch + front) * DA
        cat[at - (DA * k0 - lo):at + DA * n] = x[lo:DA * (k0 + n)]
    pick = (np.arange(len(segs))[:, None] * pitch + front + np.arange(n)[None, :])
    return cat, pick


def check_fused_bank(fmrx, oracle, mode, T, TA, N, bb, res, geo, streams, kinds, middle, tag):
    p = fmrx.modeParams(mode, T, TA)
    DA = p.audio_decim
    h_au = taps_of(fmrx, p)[2]
    junk, slot_audio, phases = geo
    na = bb // (2 * p.rf_decim * DA)
    twins = [twin_streams(fmrx, mode, T, TA, bb, streams[c], c, middle) for c in range(N)]
    n_calls = len(res["host"])
    # the models, one run per row phase over all (channel, call) segments of that phase
    want = np.zeros((n_calls, N, na), F32)
    flat = np.zeros_like(want)                       # the row0 = 0 model
    poly = np.zeros_like(want)                       # the two-kernel path's polyphase chain
    power = na >= MIN_POWER
    for ph in sorted(set(phases)):
        idx = [(k, c) for c in range(N) if phases[c] == ph for k in range(n_calls)]
        segs = [(twins[c][k][0], twins[c][k][1] * na) for k, c in idx]
        cat, pick = batch(segs, na, TA, DA)
        y = fm.fused_audio(cat, h_au, DA, row0=ph)[pick]
        # the batched run is the plain one of a segment's own stream
        x0, k0 = segs[-1]
        bits_equal(y[-1], fm.fused_audio(x0, h_au, DA, k0, na, row0=ph), tag + ": batched model")
        y0 = fm.fused_audio(cat, h_au, DA)[pick] if power and ph else y
        yp = fm.fma_chain(cat, h_au, fm.polyphase(TA, DA), DA)[pick] if power else y
        for i, (k, c) in enumerate(idx):
            want[k, c], flat[k, c], poly[k, c] = y[i], y0[i], yp[i]
    for k in range(n_calls):
        for c in range(N):
            msg = f"{tag}: call {k}, channel {c} ({kinds[c]}, row phase {phases[c]})"
            y = want[k, c]
            audio, pcm = res["host"][k]
            bits_equal(audio[c], y, msg)
            np.testing.assert_array_equal(pcm[c], oracle.pcm16(y), msg)
            for v, (want_f32, want_pcm, wrap, _) in VARIANTS.items():
                if v not in res:
                    continue
                a, s = res[v][k]
                if want_f32:
                    bits_equal(a[c], y, f"{msg}, {v}")
                if want_pcm:
                    np.testing.assert_array_equal(s[c], oracle.pcm16(y, wrap=wrap), f"{msg}, {v}")
            if power and kinds[c] == "synthetic":
                assert differs(y, poly[k, c]), msg + ": equals the two-kernel chain"
                if fm.row_phase_changes_bits(DA, phases[c]):
                    assert differs(y, flat[k, c]), msg + ": equals the row0 = 0 model"
    if N > 1:
        # channel 1: block 0 (calls 0 and 5) lies in its silence: exact zeros, out of the bank too
        assert N_BLOCKS * bb // 2 // 3 >= bb // 2
        for k in (0, n_calls - 1):
            audio, pcm = res["host"][k]
            assert not audio[1].any() and not pcm[1].any() and not want[k, 1].any(), f"{tag}: silence, call {k}"
        assert want[:, 1].any()


@pytest.mark.parametrize("T,D,TA,DA,N,kind", FUSED_BANK_CASES)
def test_fused_mono_bank(fmrx, oracle, T, D, TA, DA, N, kind):
    """The fused mono bank against fused_audio at each channel's row phase: three calls, reset of one middle channel, two
    calls, reset of the bank, the first block again; f32 + PCM from process(), PCM only (wrap, saturate) and f32 only from
    load_dev / process_dev into sentinel-filled buffers one row longer than needed."""
    mode = MODE_OF_DECIM[DA]
    p = fmrx.modeParams(mode, T, TA)
    assert (p.rf_decim, p.audio_decim) == (D, DA)
    bb = block_bytes_of(fmrx, mode, T, TA, kind)
    middle = min(N - 1, N // 2 + 1)
    streams, kinds = fused_streams(oracle, p, N, N_BLOCKS * bb // 2)
    res, geo = drive_fused(fmrx, mode, T, TA, N, bb, streams, middle, ("pcm_wrap", "pcm_saturate", "f32_only"))
    junk, slot_audio, phases = geo
    tag = f"fused bank {T}/{D}/{TA}/{DA} N {N} {kind} block ({bb} bytes, {bb // (2 * D * DA)} outputs, junk {junk})"
    print(f"{tag}: row phases met {sorted(set(phases))}")
    assert junk % 4 == 0 and slot_audio % 4 == 0 and set(phases) <= {0, 4, 8, 12}
    if kind == "smallest":
        assert bb // (2 * D * DA) < 256              # one 256-output batch of the kernel spans several slot seams
    if kind == "phases" and N >= 4:
        assert set(phases) == {0, 4, 8, 12}
    check_fused_bank(fmrx, oracle, mode, T, TA, N, bb, res, geo, streams, kinds, middle, tag)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["smallest", "phases"])
def test_fused_mono_bank_channels_are_independent(fmrx, oracle, mode, kind):
    """The handle's claim, stated directly: the same bank again with every channel but one (the weak one, between
    silence-then-full-scale and random full scale) on other streams gives that channel the same audio and PCM bits."""
    T = TA = 101
    p = fmrx.modeParams(mode, T, TA)
    N, keep = 7, 2
    bb = block_bytes_of(fmrx, mode, T, TA, kind)
    a, kinds = fused_streams(oracle, p, N, N_BLOCKS * bb // 2)
    b, _ = fused_streams(oracle, p, N, N_BLOCKS * bb // 2, salt=1)
    assert kinds[keep] == "weak" and all((a[c] != b[c]).any() for c in range(N))
    b[keep] = a[keep]
    ra, geo = drive_fused(fmrx, mode, T, TA, N, bb, a, 4)
    rb, _ = drive_fused(fmrx, mode, T, TA, N, bb, b, 4)
    print(f"fused bank mode {mode} {kind} block: row phases met {sorted(set(geo[2]))}")
    some_other = False
    for k, ((fa, sa), (fb, sb)) in enumerate(zip(ra["host"], rb["host"])):
        bits_equal(fa[keep], fb[keep], f"mode {mode} {kind} block, call {k}: channel {keep} with other neighbours")
        np.testing.assert_array_equal(sa[keep], sb[keep])
        some_other |= differs(fa[keep + 1], fb[keep + 1])
    assert some_other and any(bits(f[keep]).any() for f, _ in ra["host"])


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_mono_bank_unaligned_outputs(fmrx, oracle, mode):
    """Both output pointers one element past 16-byte alignment (include/fmrx.h promises none for this call): the scalar
    branch of channels_finish_kernel.  The bits are the model's, hence the aligned call's, and nothing outside the N rows
    is written."""
    T = TA = 101
    p = fmrx.modeParams(mode, T, TA)
    N = 7
    bb = block_bytes_of(fmrx, mode, T, TA, "phases")
    middle = 4
    streams, kinds = fused_streams(oracle, p, N, N_BLOCKS * bb // 2)
    res, geo = drive_fused(fmrx, mode, T, TA, N, bb, streams, middle, ("unaligned",))
    print(f"fused bank mode {mode}, unaligned outputs: row phases met {sorted(set(geo[2]))}")
    for k, ((fa, sa), (fu, su)) in enumerate(zip(res["host"], res["unaligned"])):
        bits_equal(fu.ravel(), fa.ravel(), f"mode {mode}, call {k}: unaligned f32 against the aligned call")
        np.testing.assert_array_equal(su, sa)
    check_fused_bank(fmrx, oracle, mode, T, TA, N, bb, res, geo, streams, kinds, middle, f"fused bank mode {mode}, unaligned outputs")


# ---- the fast mono bank of modes 2/3 -----------------------------------------------------------------------------------
def groups_per_wave(N, periods, U, stereo):
    """launch_resample's rule (kernels_bank.hip), see the module docstring.  -> (X = ceil(N / 64) periods, groups per wave)."""
    G, NW = U // 7, 3 if stereo else 7
    X = -(-N // 64) * periods
    gpw = G
    while gpw > NW and X * -(-G // gpw) * NW < 8192:
        gpw = (gpw + 1) // 2
    gpw = -(-gpw // NW) * NW
    return X, gpw // NW


def smallest_resample_block(fmrx, mode, taps, stereo=False):
    """(periods, block_bytes) of the smallest block of whole periods (U outputs <-> D IF samples) the fast bank accepts."""
    p = fmrx.modeParams(mode, 101, taps)
    for k in range(1, 64):
        bb = 2 * k * p.audio_decim * p.rf_decim
        if bb % 16:
            continue
        try:
            fmrx.Channels(mode, 1, rf_taps=101, base_audio_taps=taps, block_bytes=bb, audio_channels=2 if stereo else 1).close()
            return k, bb
        except fmrx.FmrxError as e:
            assert e.code == fmrx.EINVAL
    raise AssertionError("no block of up to 63 periods accepted")


def drive_resample_bank(fmrx, mode, taps, N, bb, calls, streams, tap_channels, pcm_only=True):
    """-> per call dict(audio [N, na], pcm [N, na], demod {c: tap}, pcm_True / pcm_False [N, na] from PCM-only calls)."""
    import torch
    mk = lambda: fmrx.Channels(mode, N, rf_taps=101, base_audio_taps=taps, block_bytes=bb)
    main = mk()
    side = {w: mk() for w in ((True, False) if pcm_only else ())}
    na = main.n_audio
    out = []
    for k in range(calls):
        iq = streams(k)
        o = main.process(iq)
        r = dict(audio=o["audio"], pcm=o["pcm16"], demod={c: main.read_tap(c, "demod") for c in tap_channels})
        if side:
            d_iq = torch.from_numpy(iq).cuda()
        for w, h in side.items():
            _, s, _, ps = device_outputs(torch, N, na, False, True)
            h.load_dev(d_iq.data_ptr())
            h.process_dev(None, ps, wrap=w)
            torch.cuda.synchronize()
            r[f"pcm_{w}"] = read_outputs(None, s, N, na, 0, f"PCM only, wrap {w}, call {k}")[1]
        out.append(r)
    for h in [main, *side.values()]:
        h.close()
    return out


@pytest.mark.parametrize("block", ["reference", "smallest"])
@pytest.mark.parametrize("N", [5, 65])
@pytest.mark.parametrize("taps", [101, 13])
@pytest.mark.parametrize("mode", [2, 3])
def test_fast_mono_bank_resampling_modes(fmrx, oracle, mode, taps, N, block):
    """chs_resample_lanes_kernel<STEREO = false> against resample_chain over the bank's own demod tap, every channel, three
    calls; 65 receivers: a second channel group with one member.  f32 + PCM, and PCM-only calls (wrap, saturate).  The demod
    tap of a subset equals the single-stream pipeline's.  Blocks of >= 1000 outputs differ from the reference's separately
    rounded order."""
    p = fmrx.modeParams(mode, 101, taps)
    U, D, calls = p.audio_upsamp, p.audio_decim, 3
    periods, bb = smallest_resample_block(fmrx, mode, taps) if block == "smallest" else (p.block_bytes // (2 * D * p.rf_decim), p.block_bytes)
    assert bb == 2 * periods * D * p.rf_decim
    X, gw = groups_per_wave(N, periods, U, False)
    print(f"fast mono bank mode {mode} taps {taps} N {N} {block} block: {periods} periods, X = {X}, {gw} group(s) per wave")
    n = calls * bb // 2
    streams = [cached_stream(oracle, c, n, p.rf_Fs) for c in range(N)]
    streams[1] = silence_then_full_scale(n, n // 3, seed=11)
    res = drive_resample_bank(fmrx, mode, taps, N, bb, calls, lambda k: np.stack([s[k * bb:(k + 1) * bb] for s in streams]), range(N))
    na, n_if = periods * U, periods * D
    h_au = taps_of(fmrx, p)[2]
    subset = sorted({0, 1, N // 2, N - 2, N - 1})
    pls = {c: fmrx.Pipeline(mode, 1, rf_taps=101, base_audio_taps=taps, max_block_bytes=bb) for c in subset}
    for c, pl in pls.items():
        pl.set_keep_intermediates(True)
        for k in range(calls):
            pl.process(streams[c][k * bb:(k + 1) * bb], want_pcm=False)
            bits_equal(res[k]["demod"][c], pl.read_tap("demod"), f"mode {mode}: bank demod vs single stream, channel {c}, call {k}")
        pl.close()
    for c in range(N):
        x = np.concatenate([r["demod"][c] for r in res])
        assert len(x) == calls * n_if
        y = fm.resample_chain(x, h_au, U, D)
        st = np.zeros(p.audio_taps - 1, F32)
        for k, r in enumerate(res):
            msg = f"fast mono bank mode {mode} taps {taps} N {N} {block} block: channel {c}, call {k}"
            yk = y[k * na:(k + 1) * na]
            bits_equal(r["audio"][c], yk, msg)
            np.testing.assert_array_equal(r["pcm"][c], oracle.pcm16(yk), msg)
            np.testing.assert_array_equal(r["pcm_True"][c], oracle.pcm16(yk, wrap=True), msg + ", PCM only, wrap")
            np.testing.assert_array_equal(r["pcm_False"][c], oracle.pcm16(yk, wrap=False), msg + ", PCM only, saturate")
            if na >= MIN_POWER and c != 1:
                ref, st = oracle.convolve_block_resample_fir(x[k * n_if:(k + 1) * n_if], h_au, st, D, U)
                assert differs(yk, ref[:na]), msg + ": equals the reference order"
        if c == 1:
            silent = (n // 3 // p.rf_decim - p.rf_taps) * U // D - p.audio_taps // U - 2
            assert silent > 0 and not y[:silent].any() and not res[0]["audio"][1][:min(silent, na)].any()


def base_streams(oracle, p, n_samples):
    s = [cached_stream(oracle, b, n_samples, p.rf_Fs) for b in range(16)]
    s[1] = silence_then_full_scale(n_samples, n_samples // 3, seed=11)
    return np.stack(s)


def multi_group_subset(N):
    """Channels 0, 63, 64, the last one, and the two ends of the last full group of 64."""
    full = N // 64 * 64
    return sorted({0, 63, 64, full - 64, full - 1, N - 1})


@pytest.mark.parametrize("X_min,want_groups", [(147, 2), (294, 3)])
def test_fast_mono_bank_several_groups_per_wave(fmrx, oracle, X_min, want_groups):
    """Mono mode 3 at X = ceil(N / 64) periods >= 147 (>= 293: 294, the first multiple of 7): every wave walks 2 (3) groups of 7 outputs, reusing its
    wave-private staging area without a barrier.  One reference block of 7 periods per call: N = 64 X_min / 7 - 44 receivers
    (the last channel group is not full) on 16 base streams.  Channels 0 .. 15 and the subset against the model; every
    channel bit for bit against the first channel of its base stream."""
    mode, taps, calls = 3, 101, 2
    p = fmrx.modeParams(mode, 101, taps)
    U, D, bb = p.audio_upsamp, p.audio_decim, p.block_bytes
    periods = bb // (2 * D * p.rf_decim)
    assert periods == 7 and X_min % periods == 0
    N = 64 * X_min // periods - 44
    X, gw = groups_per_wave(N, periods, U, False)
    assert X == X_min and gw == want_groups and groups_per_wave(N - 64, periods, U, False)[1] == want_groups - 1
    print(f"fast mono bank mode {mode}, {N} receivers x {periods} periods: X = {X}, {gw} groups per wave")
    base = base_streams(oracle, p, calls * bb // 2)
    of = np.arange(N) % 16
    subset = multi_group_subset(N)
    res = drive_resample_bank(fmrx, mode, taps, N, bb, calls, lambda k: base[of, k * bb:(k + 1) * bb], sorted(set(range(16)) | set(subset)),
                              pcm_only=False)
    check_against_base_streams(oracle, res, fm_model=lambda x: fm.resample_chain(x, taps_of(fmrx, p)[2], U, D), N=N, subset=subset,
                               na=periods * U, tag=f"mono mode 3, {N} receivers")


def check_against_base_streams(oracle, res, fm_model, N, subset, na, tag):
    of = np.arange(N) % 16
    model = {}
    for b in range(16):
        model[b] = fm_model(np.concatenate([r["demod"][b] for r in res]))
    for k, r in enumerate(res):
        a, s = bits(r["audio"]), r["pcm"]
        bad = np.flatnonzero((a != a[of]).any(axis=1) | (s != s[of]).any(axis=1))
        assert len(bad) == 0, f"{tag}, call {k}: channels {bad[:8]} differ from the first channel of their base stream"
        for c in sorted(set(range(16)) | set(subset)):
            msg = f"{tag}: channel {c}, call {k}"
            bits_equal(r["demod"][c], r["demod"][c % 16], msg + ": demod tap")
            y = model[c % 16][k * na:(k + 1) * na]
            bits_equal(r["audio"][c], y, msg)
            np.testing.assert_array_equal(r["pcm"][c], oracle.pcm16(y), msg)
    assert len({r["audio"][b].tobytes() for b in range(16)}) == 16


def test_fast_stereo_bank_several_groups_per_wave(fmrx, oracle):
    """Stereo mode 3 at X >= 171: every wave of chs_resample_lanes_kernel<STEREO = true> walks 2 groups.  A stereo call runs
    in up to 8 chunks of whole periods and launches the resampler once per chunk, so X counts the periods of a chunk: the
    smallest block the bank accepts (ceil(periods / 8) periods per chunk), and
    N = 64 * 171 / (periods per chunk) - 30 receivers on 16 base streams.  The model is that of
    tests/test_gpu_fir_exact.py's test_fast_stereo_bank_resampling_modes, fed the bank's demod, stereo_filt and pll taps."""
    mode, taps, calls = 3, (101, 101, 101), 3
    p = fmrx.modeParams(mode, *taps)
    U, D = p.audio_upsamp, p.audio_decim
    periods, bb = smallest_resample_block(fmrx, mode, taps[1], stereo=True)
    per_chunk = -(-periods // 8)
    assert per_chunk == 1
    N = 64 * 171 // per_chunk - 30
    X, gw = groups_per_wave(N, per_chunk, U, True)
    assert X == 171 and gw == 2 and groups_per_wave(N - 64, per_chunk, U, True)[1] == 1
    print(f"fast stereo bank mode {mode}, {N} receivers x {periods} period(s) per call, {per_chunk} per chunk: X = {X}, {gw} groups per wave")
    base = base_streams(oracle, p, calls * bb // 2)
    of = np.arange(N) % 16
    subset = multi_group_subset(N)
    tapped = sorted(set(range(16)) | set(subset))
    ch = fmrx.Channels(mode, N, rf_taps=taps[0], base_audio_taps=taps[1], stereo_taps=taps[2], audio_channels=2, exact=False, block_bytes=bb)
    res = []
    for k in range(calls):
        o = ch.process(base[of, k * bb:(k + 1) * bb])
        r = {t: {c: ch.read_tap(c, t) for c in tapped} for t in ("demod", "stereo_filt", "pll")}
        r.update(audio=o["audio"], pcm=o["pcm16"])
        res.append(r)
    ch.close()
    h_st, _, h_au = taps_of(fmrx, p)
    delay, na = (p.stereo_taps - 1) // 2, periods * U
    model = {}
    for b in range(16):
        x = np.concatenate([r["demod"][b] for r in res])
        sf = fm.fma_chain(x, h_st, fm.ascending(p.stereo_taps))
        mix = np.concatenate([fm.mixer(r["stereo_filt"][b], r["pll"][b]) for r in res])
        model[b] = (sf, fm.combine(fm.resample_chain(mix, h_au, U, D), fm.resample_chain(x, h_au, U, D, delay)))
    n_if = periods * D
    for k, r in enumerate(res):
        a, s = bits(r["audio"]).reshape(N, -1), r["pcm"].reshape(N, -1)
        bad = np.flatnonzero((a != a[of]).any(axis=1) | (s != s[of]).any(axis=1))
        assert len(bad) == 0, f"stereo mode 3, call {k}: channels {bad[:8]} differ from the first channel of their base stream"
        for c in tapped:
            msg = f"stereo mode 3, {N} receivers: channel {c}, call {k}"
            for t in ("demod", "stereo_filt", "pll"):
                bits_equal(r[t][c], r[t][c % 16], f"{msg}: {t} tap")
            sf, (left, right) = model[c % 16]
            bits_equal(r["stereo_filt"][c], sf[k * n_if:(k + 1) * n_if], msg + ": stereo_filt")
            bits_equal(r["audio"][c, 0], left[k * na:(k + 1) * na], msg + ": left")
            bits_equal(r["audio"][c, 1], right[k * na:(k + 1) * na], msg + ": right")
            np.testing.assert_array_equal(r["pcm"][c, :, 0], oracle.pcm16(left[k * na:(k + 1) * na]), msg)
            np.testing.assert_array_equal(r["pcm"][c, :, 1], oracle.pcm16(right[k * na:(k + 1) * na]), msg)
    assert len({r["audio"][b].tobytes() for b in range(16)}) == 16
