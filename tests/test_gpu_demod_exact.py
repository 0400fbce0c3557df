"""The fast FM discriminator (csrc/device_math.hpp: demod_fast, demod_fast_bounded) checked BIT FOR BIT, sample by sample,
at every place it is written out, against tests/_demod_model.py given the one thing a host cannot restate: the device's own
v_rcp_f32 of den*sc, read through the rcp hook (fmrx.deviceRcp).  num, den, the 2^-60 / 2^64 scaling, the product with the
reciprocal and the den == 0 select are the model's; so a contracted product, a wrong previous sample at a lane, tile, wave or
block seam, a scaling that differs between the two forms or a denormal reaching the reciprocal changes bits here, where the
RMS bound of test_gpu_parity.py's test_front_end_matrix_core_kernel sees nothing.

The six sites and the case that reaches each:
  1. demod_fast, demod_fast_bounded themselves          test_hook_* (fmrx.fmDemodFast = demod_if_kernel<1>, <2>): free operands
  2. fe_mfma_kernel, general loop (demod_fast)           test_pipeline_streams[mfma-*]: D = 10 everywhere; D < 10 on the first P
                                                         and the last tiles of a wave, ragged last tiles, the smallest blocks
     fe_mfma_kernel, straight-line tiles                 test_pipeline_steady_block[mfma-*] (modes 1, 3: D = 5, 3), keep_intermediates
     (demod_fast_bounded, MODE 3 and MODE 1)             on (MODE 3) and off (MODE 1)
  3. fe_mfma_bank_kernel                                 test_fast_banks: stereo banks of modes 0, 1, mono banks of modes 2, 3
  4. mono_fused_kernel, general tiles and                test_fused_mono_on_the_weak_stream: small blocks (general tiles) and a
     straight-line batches (demod_fast_bounded)          block of more batches than waves (straight-line), through the audio FIR
  5. fe_demod_kernel's packed-pair restatement           test_pipeline_streams[valu-*], test_pipeline_steady_block[valu-*]
  6. demod_if_kernel<FAST>                               the hook of site 1 is this kernel
The previous IF sample comes by __shfl (2, 3), __shfl_up (5), register carries (4) or prev_override after set_state (2, 5:
test_pipeline_streams' cut runs restore the state before every block, test_prev_override_is_read sets a pair the history does
not explain).

A build whose demod_fast_bounded contracts its numerator to an fma fails test_hook_free_operands, test_hook_degenerate_operands,
test_pipeline_steady_block[mfma-*] and test_fused_mono_on_the_weak_stream, and passes test_front_end_matrix_core_kernel.

The premise -- v_rcp_f32 is within 1 ulp and works on the mantissa alone -- is test_rcp_*; where the hardware steps outside it
the failure message carries the operands."""
import numpy as np
import pytest

import _demod_model as dm
import _fe_model as fe
from test_gpu_channels import channel_stream
from test_gpu_fe_exact import mf_cfg
from test_gpu_fir_exact import taps_of
from test_gpu_mfma_exact import check_fused, run_fused

pytestmark = pytest.mark.gpu

F, U8 = np.float32, np.uint8
MFMA_SEAM = 120            # outputs per tile of the matrix-core kernels (MfCfg::TILE_OUT)
VALU_SEAM = 63 * 8         # FeWaveCfg<T, D, 8>::STRIDE: new outputs per wave tile of fe_demod_kernel


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def assert_bits(got, want, msg, ctx=None):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size:
        k = bad[:4]
        extra = "" if ctx is None else "; operands " + repr({n: np.asarray(v)[k].tolist() for n, v in ctx.items()})
        raise AssertionError(f"{msg}: {bad.size} of {got.size} differ, first at {bad[:8].tolist()}: got {got[k].tolist()} "
                             f"({[hex(v) for v in bits(got)[k]]}) want {want[k].tolist()} ({[hex(v) for v in bits(want)[k]]}){extra}")


def model(fmrx, I, Q, pi, pq):
    """The kernel's answer: the model's parts with the device's own reciprocal of den*sc."""
    p = dm.parts(I, Q, pi, pq)
    return dm.exact_given_rcp(p, fmrx.deviceRcp(p.ds)), p


def check_demod(fmrx, got, I, Q, prev, msg, need_normal=True):
    """got against the model of the IF (I, Q), the sample in front of it being prev; -> the parts."""
    pi, pq = dm.previous(I, Q, *prev)
    want, p = model(fmrx, I, Q, pi, pq)
    if need_normal:
        ok = dm.all_zero_or_normal(p)
        assert ok.all(), (msg, "the stream reaches a denormal intermediate", int((~ok).sum()))
    assert_bits(got, want, msg, dict(i=I, q=Q, pi=pi, pq=pq))
    return p


# ---- a. the premise: the reciprocal ------------------------------------------------------------------------------------------
def test_rcp_of_every_mantissa_is_within_one_ulp(fmrx):
    """rcp(x) for every float32 in [1, 2) -- all 2^23 mantissas -- is RN(1/x) or one of its two neighbours."""
    x = (np.arange(1 << 23, dtype=np.uint32) + np.uint32(0x3F800000)).view(F)
    r = fmrx.deviceRcp(x)
    ok = np.zeros(x.shape, bool)
    for c in dm.rcp_candidates(x):
        ok |= bits(r) == bits(c)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"v_rcp_f32 outside RN(1/x) +- 1 ulp on {bad.size} mantissas, first x = {x[bad[:4]].tolist()} "
                           f"rcp = {r[bad[:4]].tolist()} RN = {dm.rcp_rn(x[bad[:4]]).tolist()}")
    exact = float(np.mean(bits(r) == bits(dm.rcp_rn(x))))
    print(f"v_rcp_f32 on [1, 2): correctly rounded on {exact:.4%} of the mantissas")
    assert bits(r[:1])[0] == 0x3F800000                       # rcp(1) = 1


def test_rcp_works_on_the_mantissa_alone(fmrx):
    """rcp(m 2^e) == rcp(m) 2^-e exactly, 4096 random mantissas at every normal exponent whose result is normal (e = -126 .. 125;
    m = 1 reaches 2^126) -- what makes the 2^64 scaling of demod_fast invisible in the result -- and both signs."""
    rng = np.random.default_rng(21)
    es = np.arange(-126, 126)
    m = (rng.integers(0, 1 << 23, (len(es), 4096), dtype=np.uint32) + np.uint32(0x3F800000)).view(F)
    m[:, 0] = 1.0
    x = np.ldexp(m, es[:, None].astype(np.int32)).astype(F)
    x[:, 1::2] *= F(-1.0)
    want = np.ldexp(fmrx.deviceRcp(np.abs(m).reshape(-1)).reshape(m.shape), -es[:, None].astype(np.int32)).astype(F)
    want[:, 1::2] *= F(-1.0)
    got = fmrx.deviceRcp(x.reshape(-1)).reshape(x.shape)
    assert np.all(np.abs(want) >= dm.TINY) and np.all(np.isfinite(want))
    assert_bits(got.reshape(-1), want.reshape(-1), "rcp(m 2^e) != rcp(m) 2^-e", dict(x=x.reshape(-1)))


# ---- b. the hook on free operands --------------------------------------------------------------------------------------------
def hook(fmrx, I, Q, prev=(0.0, 0.0), bounded=False):
    return fmrx.fmDemodFast(I, Q, prev[0], prev[1], bounded=bounded)


def free_streams(rng, n):
    """name -> (I, Q, prev): each output k uses pair k and pair k - 1, so a random stream is n free operand quadruples."""
    out = {}
    out["standard normals"] = (rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F), (0.3, -0.2))
    # |z| from 2^-52 to 2^-20: den crosses 2^-60 from both sides, every intermediate normal (below 2^-52 the squares and
    # products go denormal: test_hook_tiny_operands_and_the_reference_contract sweeps 2^-78 .. 2^-50)
    e = np.repeat(np.linspace(-52, -20, n // 2), 2)
    th = rng.uniform(0.1, np.pi / 2 - 0.1, n) + rng.integers(0, 4, n) * (np.pi / 2)
    out["|z| 2^-52 .. 2^-20"] = ((np.exp2(e) * np.cos(th)).astype(F), (np.exp2(e) * np.sin(th)).astype(F), (2.0 ** -40, 0.0))
    # den exactly 2^-60, just below and just above, from one-component pairs (I^2 exact)
    one = np.array([2.0 ** -30, np.nextafter(F(2.0 ** -30), F(0)), np.nextafter(F(2.0 ** -30), F(1)), -2.0 ** -30] * 8, F)
    out["den at 2^-60"] = (one, np.zeros_like(one), (2.0 ** -31, 2.0 ** -31))
    out["den at 2^-60, on Q"] = (np.zeros_like(one), one, (2.0 ** -31, -2.0 ** -31))
    # full scale: the largest IF a byte stream can give is sum|h| < 2; and far beyond it
    fs = rng.choice(np.array([1.0, -1.0, 2.0 - 2.0 ** -23, -(2.0 - 2.0 ** -23), 127.0 / 128, -1.0 / 128, 1e3, -1e6], F), (2, n))
    out["full scale"] = (fs[0].copy(), fs[1].copy(), (1.0, -1.0))
    return out


def test_hook_free_operands(fmrx):
    """fmDemodFast (demod_if_kernel<1>: demod_fast) on free operands whose every intermediate is zero or normal: bit-equal to
    the model with the device's reciprocal; bounded = 1 (demod_fast_bounded) the same bits wherever the operands are 0 or
    >= 2^-50 in magnitude -- den in [2^-100, 2^-60) included, where one form scales and the other does not."""
    rng = np.random.default_rng(22)
    seen_scaled_bounded = False
    for name, (I, Q, prev) in free_streams(rng, 1 << 16).items():
        got = hook(fmrx, I, Q, prev)
        p = check_demod(fmrx, got, I, Q, prev, f"demod_fast, {name}")
        pi, pq = dm.previous(I, Q, *prev)
        big = np.ones(len(I), bool)
        for v in (I, Q, pi, pq):
            big &= (v == 0) | (np.abs(v) >= F(2.0 ** -50))
        gb = hook(fmrx, I, Q, prev, bounded=True)
        assert_bits(gb[big], got[big], f"demod_fast_bounded != demod_fast, {name}", dict(i=I[big], q=Q[big], pi=pi[big], pq=pq[big]))
        seen_scaled_bounded |= bool((big & (p.den != 0) & (p.den < dm.THRESHOLD)).any())
        if name.startswith("den at"):
            assert (p.den == dm.THRESHOLD).any() and (p.den < dm.THRESHOLD).any() and (p.den > dm.THRESHOLD).any()
            assert (p.sc[p.den == dm.THRESHOLD] == 1).all()
    assert seen_scaled_bounded


def test_hook_degenerate_operands(fmrx):
    """den == 0 from every combination of +-0 operands and previous samples (finite, huge, tiny): the bit pattern of +0.0, both
    forms.  Previous = (0, 0): I*Q - Q*I cancels exactly, +0.0 for every den != 0.  z equal to its previous: 0."""
    rng = np.random.default_rng(23)
    z = np.array([0.0, -0.0], F)
    I = np.tile(np.repeat(z, 2), 64)
    Q = np.tile(np.tile(z, 2), 64)
    # the previous pair of output k is pair k - 1: interleave zero pairs with arbitrary ones and look at the zero pairs
    n = len(I)
    Ii, Qi = np.empty(2 * n, F), np.empty(2 * n, F)
    Ii[1::2], Qi[1::2] = I, Q
    Ii[0::2] = rng.choice(np.array([0.0, -0.0, 1.0, -3e38, 1e-45, 2.0 ** -70], F), n)
    Qi[0::2] = rng.choice(np.array([0.0, -0.0, -1.0, 3e38, -1e-45, 2.0 ** -70], F), n)
    for bounded in (False, True):
        got = hook(fmrx, Ii, Qi, (0.0, -0.0), bounded)
        assert not bits(got[1::2]).any(), ("den == 0 must give +0.0", bounded, got[1::2][bits(got[1::2]) != 0][:4].tolist())
    # previous = (0, 0): pairs (z, 0, z, 0, ...) -- every odd output has a zero pair in front of it
    m = 1 << 15
    Ii, Qi = np.zeros(2 * m, F), np.zeros(2 * m, F)
    e = rng.uniform(-30, 1, m)
    Ii[1::2] = (rng.standard_normal(m) * np.exp2(e)).astype(F)
    Qi[1::2] = (rng.standard_normal(m) * np.exp2(e)).astype(F)
    for bounded in (False, True):
        got = hook(fmrx, Ii, Qi, (0.0, 0.0), bounded)
        assert not bits(got).any(), ("I*Q - Q*I must be +0.0", bounded, np.flatnonzero(bits(got))[:8].tolist())
    check_demod(fmrx, hook(fmrx, Ii, Qi), Ii, Qi, (0.0, 0.0), "previous = (0, 0)")
    # z equal to its previous sample: runs of a repeated pair
    Ir = np.repeat((rng.standard_normal(m // 4) * np.exp2(e[:m // 4])).astype(F), 4)
    Qr = np.repeat((rng.standard_normal(m // 4) * np.exp2(e[:m // 4])).astype(F), 4)
    for bounded in (False, True):
        got = hook(fmrx, Ir, Qr, (Ir[0], Qr[0]), bounded)
        rep = np.ones(len(Ir), bool)
        rep[4::4] = False
        assert not got[rep].any(), ("a constant IF must give 0", bounded)
    check_demod(fmrx, hook(fmrx, Ir, Qr, (Ir[0], Qr[0])), Ir, Qr, (Ir[0], Qr[0]), "z == previous")


def test_hook_tiny_operands_and_the_reference_contract(fmrx, oracle):
    """|z| from 2^-78 to 2^-50: squares, products and den are float32 denormals below 2^-63 and underflow to zero below 2^-75.  The exact
    stage (fmDemod) equals the oracle there, denormal den included: the reference contract.  The fast form against the model's
    stated rule -- denormals KEPT by every multiply and add; the reciprocal sees den 2^64, a normal number.  (Unreachable from
    the pipeline: test_pipeline_streams asserts that its streams keep every intermediate zero or normal.)"""
    rng = np.random.default_rng(24)
    n = 1 << 16
    e = np.repeat(np.linspace(-78, -50, n // 2), 2)
    th = rng.uniform(0, 2 * np.pi, n)
    I, Q = (np.exp2(e) * np.cos(th)).astype(F), (np.exp2(e) * np.sin(th)).astype(F)
    prev = (2.0 ** -64, -2.0 ** -66)
    want, _, _ = oracle.fm_demod(I, Q, *prev)
    assert_bits(fmrx.fmDemod(I, Q, *prev)[0], want, "fmDemod on tiny operands", dict(i=I, q=Q))
    pi, pq = dm.previous(I, Q, *prev)
    p = dm.parts(I, Q, pi, pq)
    den_denormal = (p.den > 0) & (p.den < dm.TINY)
    assert den_denormal.any() and (p.den == 0).any() and ((np.abs(p.a) > 0) & (np.abs(p.a) < dm.TINY)).any()
    assert (p.ds[den_denormal] >= dm.TINY).all()              # scaled: what the reciprocal sees is normal
    check_demod(fmrx, hook(fmrx, I, Q, prev), I, Q, prev, "demod_fast on denormal intermediates (model: denormals kept)",
                need_normal=False)


# ---- c. every kernel site ------------------------------------------------------------------------------------------------------
def weak_bytes(rng, n_bytes, density=1 / 32):
    """Silence with sparse 127 / 129 bytes: IF samples a few units of 2^-(s+7), den tiny."""
    s = np.full(n_bytes, 128, U8)
    hit = rng.random(n_bytes) < density
    s[hit] = rng.choice(np.array([127, 129], U8), int(hit.sum()))
    return s


def impulses(s, samples):
    """One 0 byte on one channel and one 255 byte on the other at each of the given samples (alternating which)."""
    for j, p in enumerate(samples):
        if 0 <= p < len(s) // 2:
            s[2 * p + (j & 1)], s[2 * p + 1 - (j & 1)] = 0, 255


def tiny_pattern(q, lim=3, amps=(1, 2, 3)):
    """Three taps and byte offsets x (|x| <= 3) with 0 < |sum q[tap] x| <= lim units of the IF grid: sparse bytes in silence
    that cancel to an IF sample below 2^-30, so that den < 2^-60 -- the range in which demod_fast scales and
    demod_fast_bounded does not.  (A single byte cannot: the smallest nonzero designed tap is tens of units.)  q: the integer
    taps of tests/_fe_model.py.  -> [(tap, x)] or None where the taps allow none (13 taps)."""
    vals, meta = [], []
    for a in np.flatnonzero(q != 0):
        for x in amps:
            for sg in (1, -1):
                vals.append(int(q[a]) * x * sg)
                meta.append((int(a), x * sg))
    vals, meta = np.array(vals, np.int64), np.array(meta, np.int64)
    i, j = np.triu_indices(len(vals), 1)
    ok = meta[i, 0] != meta[j, 0]
    i, j = i[ok], j[ok]
    ps = vals[i] + vals[j]
    order = np.argsort(ps, kind="stable")
    ps = ps[order]
    best = None
    for v, (t, x) in zip(vals, meta):
        pos = int(np.searchsorted(ps, -v))
        for pp in range(max(0, pos - 3), min(len(ps), pos + 3)):
            k, tot = order[pp], abs(int(ps[pp] + v))
            if 0 < tot <= lim and t not in (meta[i[k], 0], meta[j[k], 0]) and (best is None or tot < best[0]):
                best = (tot, [tuple(meta[i[k]].tolist()), tuple(meta[j[k]].tolist()), (int(t), int(x))])
    return best and best[1]


def plant(s, n, pat, q, T, D):
    """Silence around sample n (a multiple of D: an output), then the pattern on I and its negative on Q so that output n is
    (+-tiny, -+tiny), and one more byte on Q that only the output in front sees (tap index >= T - D there, past the window of
    output n), so that the previous pair is not on the same line through 0 and num != 0."""
    lo, hi = max(0, n - T - D), min(len(s) // 2, n + T + D)
    s[2 * lo:2 * hi] = 128
    for t, x in pat:
        if n - t >= 0:
            s[2 * (n - t)], s[2 * (n - t) + 1] = 128 + x, 128 - x
    live = [t for t in range(T - D, T) if q[t] != 0]
    if live and n - D - live[0] >= 0:
        s[2 * (n - D - live[0]) + 1] = 129


def quantised_taps(h):
    return fe.fe_digits(h, fe.fe_scale(h))[0]


def composite(oracle, rng, p, cuts, seam, T, h):
    """One stream of sum(cuts) bytes.  First 55 %: the weak stream, with isolated 0 / 255 impulses at the first and last sample
    of every block that starts there (cuts, bytes), on both sides of the tile seams behind each such block's start (and behind
    the stream's start: the one-block run's seams) and in the middle of the next block's history; and tiny_pattern planted at a
    tile's first output, at a block's second tile and mid-tile.  Then silence followed by a constant byte pair, random 0 / 255
    bytes, and the synthetic FM stream."""
    D, n_bytes = p.rf_decim, sum(cuts)
    a, b, c = int(n_bytes * 0.55) // 16 * 16, int(n_bytes * 0.70) // 16 * 16, int(n_bytes * 0.85) // 16 * 16
    s = weak_bytes(rng, n_bytes)
    spots, off = [], 0
    for nb in cuts:
        if off < a:
            k0, k1 = off // 2, (off + nb) // 2
            spots += [k0, k1 - 1, k1 - 1 - (T - 1) // 2]
            for t in range(1, 4):
                spots += [k0 + seam * t * D + d for d in (-1, 0, 1)]
        off += nb
    for t in range(1, a // 2 // (seam * D), max(1, a // 2 // (seam * D) // 6)):
        spots += [seam * t * D + d for d in (-1, 0, 1)]
    spots = sorted({q for q in spots if 0 <= q < a // 2})
    for q in spots:                                          # isolated: silence around each impulse
        s[max(0, 2 * q - 8):2 * q + 10] = 128
    impulses(s, spots)
    pat, q = tiny_pattern(quantised_taps(h)), quantised_taps(h)
    if pat:
        off = 0
        for nb in cuts[:5]:
            k0 = off // 2
            for n in (k0 + 2 * seam * D, k0 + (3 * seam + seam // 2 + 1) * D):
                if k0 + T + D < n and n + T + D < min(a, off + nb) // 2:
                    plant(s, n, pat, q, T, D)
            off += nb
    s[a:b] = 128
    s[a + (b - a) // 2:b:2], s[a + (b - a) // 2 + 1:b:2] = 131, 120
    s[b:c] = rng.integers(0, 2, c - b).astype(U8) * 255
    s[c:] = channel_stream(oracle, 5, (n_bytes - c) // 2, p.rf_Fs)
    return s


def smallest_block(fmrx, mode, T, unit):
    """The smallest multiple of `unit` bytes the pipeline accepts, found by asking it."""
    pl = fmrx.Pipeline(mode, 1, rf_taps=T, base_audio_taps=13, max_block_bytes=64 * unit)
    try:
        for k in range(1, 65):
            try:
                pl.process(np.full(k * unit, 128, U8), want_pcm=False)
                return k * unit
            except fmrx.FmrxError:
                continue
    finally:
        pl.close()
    raise AssertionError("no block of up to 64 units accepted")


def pipeline_unit(p):
    A, Uu = p.audio_decim, max(p.audio_upsamp, 1)
    return int(2 * p.rf_decim * np.lcm(A // np.gcd(A, Uu), 8))      # bytes: whole audio periods, 16-byte multiples


def run_pipeline(fmrx, mode, T, variant, keep, blocks, restore_state=False, prev_patch=None):
    """-> per block dict(demod, if_i, if_q (keep only)).  restore_state: get_state / set_state in front of every block but the
    first, so that the kernel takes its previous IF sample from the carried pair (prev_override).  The fused mono kernel is
    switched off (its discriminator stays on chip: test_fused_mono_on_the_weak_stream): the front-end kernels run at any size."""
    pl = fmrx.Pipeline(mode, 1, rf_taps=T, base_audio_taps=13, max_block_bytes=max(len(b) for b in blocks))
    pl.set_option("fe_variant", variant)
    pl.set_option("fused_min_audio", 10 ** 12)
    pl.set_keep_intermediates(keep)
    out = []
    for k, blk in enumerate(blocks):
        if restore_state and k:
            st = pl.get_state()
            if prev_patch is not None:
                st[2 * (T - 1):2 * (T - 1) + 2] = prev_patch
            pl.set_state(st)
        pl.process(blk, want_pcm=False)
        r = dict(demod=pl.read_tap("demod"))
        if keep:
            r.update(if_i=pl.read_tap("if_i"), if_q=pl.read_tap("if_q"))
        out.append(r)
    pl.close()
    return out


def cut(stream, cuts):
    out, o = [], 0
    for c in cuts:
        out.append(stream[o:o + c])
        o += c
    assert o == len(stream)
    return out


def cat(res, key):
    return np.concatenate([r[key] for r in res])


@pytest.mark.parametrize("T", [13, 101, 151])
@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("variant", ["mfma", "valu"])
def test_pipeline_streams(fmrx, oracle, variant, mode, T):
    """The single-stream pipeline's discriminator (fe_mfma_kernel / fe_demod_kernel), D = 10, 5, 3 x rf taps 13, 101, 151, on the
    composite stream: in cuts -- the smallest block the pipeline accepts, a ragged last tile, blocks of several tiles -- with
    the state restored in front of every block (prev_override), keep_intermediates on and off; and as ONE block.  The demod tap
    is bit-equal to the model of the if_i / if_q taps (the first sample's previous pair: the block before's last, zeros at the
    start); with keep_intermediates off it is bit-equal to the twin's that kept them; the one-block run gives the cut runs'
    bits.  mfma: the IF taps are the integer model's (tests/_fe_model.py); valu: they differ from it (the other kernel ran)."""
    p = fmrx.modeParams(mode, T, 13)
    D, unit = p.rf_decim, pipeline_unit(p)
    seam = MFMA_SEAM if variant == "mfma" else VALU_SEAM
    small = smallest_block(fmrx, mode, T, unit)
    up = lambda nb: -(-nb // unit) * unit
    ragged = up(2 * D * (3 * seam + 7))                      # three tiles and a few outputs of a fourth
    cuts = [up(2 * D * (5 * seam + 61)), small, ragged, small, up(2 * D * (9 * seam + 1)), up(2 * D * 4 * seam), small, ragged]
    rng = np.random.default_rng(1000 * mode + 10 * T + (variant == "valu"))
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, T)
    stream = composite(oracle, rng, p, cuts, seam, T, h)
    tag = f"{variant} mode {mode} taps {T}"

    kept = run_pipeline(fmrx, mode, T, variant, True, cut(stream, cuts), restore_state=True)
    prev, normal_den = (0.0, 0.0), []
    for b, r in enumerate(kept):
        parts = check_demod(fmrx, r["demod"], r["if_i"], r["if_q"], prev, f"{tag}, block {b} ({cuts[b]} bytes)")
        normal_den.append(parts.den)
        prev = (r["if_i"][-1], r["if_q"][-1])
    den = np.concatenate(normal_den)
    assert (den == 0).any() and (den > 0.01).any() and den[den > 0].min() < 1e-6                  # silent, loud and weak samples
    scaled = int(((den > 0) & (den < dm.THRESHOLD)).sum())
    print(f"{tag}: {scaled} samples with 0 < den < 2^-60, smallest nonzero den {den[den > 0].min():.3e}")
    if variant == "mfma" and T > 13:                         # (13 taps allow no pattern; the valu kernel's IF is not on the grid)
        assert scaled >= 2, tag

    mi, mq = fe.fe_model(stream, np.full(2 * (T - 1), 128, U8), h, D)
    if variant == "mfma":
        assert_bits(cat(kept, "if_i"), mi, tag + ": if_i against the integer model")
        assert_bits(cat(kept, "if_q"), mq, tag + ": if_q against the integer model")
    else:
        assert (bits(cat(kept, "if_i")) != bits(mi)).any(), tag + ": the IF equals the matrix-core kernel's"

    lean = run_pipeline(fmrx, mode, T, variant, False, cut(stream, cuts), restore_state=True)
    assert_bits(cat(lean, "demod"), cat(kept, "demod"), tag + ": keep_intermediates off against the twin that kept its IF")
    for keep in (True, False):
        whole = run_pipeline(fmrx, mode, T, variant, keep, [stream])
        assert_bits(whole[0]["demod"], cat(kept, "demod"), f"{tag}: one block (keep {keep}) against the cuts")
        if keep:
            assert_bits(whole[0]["if_i"], cat(kept, "if_i"), tag + ": one block, if_i")
            assert_bits(whole[0]["if_q"], cat(kept, "if_q"), tag + ": one block, if_q")


@pytest.mark.parametrize("variant", ["mfma", "valu"])
def test_prev_override_is_read(fmrx, oracle, variant):
    """set_state with a previous IF pair that the byte history does not explain: the first output of the next block is the model's
    with THAT pair, a weak one and a loud one (prev_override in fe_mfma_kernel / fe_demod_kernel)."""
    mode, T = 1, 101
    p = fmrx.modeParams(mode, T, 13)
    nb = -(-2 * p.rf_decim * 300 // pipeline_unit(p)) * pipeline_unit(p)
    rng = np.random.default_rng(31)
    stream = weak_bytes(rng, 2 * nb, density=1 / 8)
    for patch in ((F(5 * 2.0 ** -33), F(-3 * 2.0 ** -33)), (F(0.25), F(-0.75))):
        res = run_pipeline(fmrx, mode, T, variant, True, cut(stream, [nb, nb]), restore_state=True, prev_patch=patch)
        r = res[1]
        assert r["if_i"][0] != 0 or r["if_q"][0] != 0
        check_demod(fmrx, r["demod"], r["if_i"], r["if_q"], patch, f"{variant}: previous pair {patch} from set_state")
        other = dm.previous(r["if_i"], r["if_q"], res[0]["if_i"][-1], res[0]["if_q"][-1])
        assert bits(model(fmrx, r["if_i"], r["if_q"], *other)[0])[0] != bits(r["demod"])[0]   # (the history's pair gives another)


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("variant", ["mfma", "valu"])
def test_pipeline_steady_block(fmrx, oracle, variant, mode):
    """One block of the size tests/test_gpu_fe_exact.py uses to put every wave of the matrix-core kernel's full grid past its
    ramp-up: (3P + 4) tiles of 120 D samples for each of the grid's `waves` waves (mf_cfg), 3P + 4 >= 2 (P + 1), so the
    straight-line tiles (demod_fast_bounded, D < 10) run on most of it -- MODE 3 with keep_intermediates on, MODE 1 with it
    off (the fused mono kernel, which mode 1 would take at this size, is switched off).  The same
    block gives every wave of fe_demod_kernel's grid (at most 4096 waves, 504 outputs a tile) two tiles or more.  First half
    weak (den in the range where only demod_fast scales), second half random 0 / 255 bytes."""
    T = 101
    p = fmrx.modeParams(mode, T, 13)
    D, unit = p.rf_decim, pipeline_unit(p)
    P, waves = mf_cfg(T, D)
    nb = -(-2 * (3 * P + 4) * waves * MFMA_SEAM * D // unit) * unit
    assert nb // (2 * D) >= 2 * 4096 * VALU_SEAM
    rng = np.random.default_rng(40 + mode)
    blk = weak_bytes(rng, nb)
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, T)
    q = quantised_taps(h)
    pat = tiny_pattern(q)
    assert pat
    for n in range(700 * D, nb // 4 - 2 * T, 1501 * D):      # tiny IF samples all over the weak half, every place in a tile
        plant(blk, n, pat, q, T, D)
    blk[nb // 2:] = rng.integers(0, 2, nb - nb // 2).astype(U8) * 255
    kept = run_pipeline(fmrx, mode, T, variant, True, [blk])[0]
    parts = check_demod(fmrx, kept["demod"], kept["if_i"], kept["if_q"], (0.0, 0.0), f"{variant} mode {mode}, {nb} bytes, keep on")
    scaled = int(((parts.den >= F(2.0 ** -100)) & (parts.den < dm.THRESHOLD)).sum())
    print(f"{variant} mode {mode}: {scaled} samples with 2^-100 <= den < 2^-60")
    if variant == "mfma":                                     # (the valu kernel's IF is not on the integer grid)
        assert scaled >= 1000
    lean = run_pipeline(fmrx, mode, T, variant, False, [blk])[0]
    assert_bits(lean["demod"], kept["demod"], f"{variant} mode {mode}, {nb} bytes, keep off against the twin")


@pytest.mark.parametrize("mode,audio_channels", [(0, 2), (1, 2), (2, 1), (3, 1)])
def test_fast_banks(fmrx, oracle, mode, audio_channels):
    """fe_mfma_bank_kernel behind Channels(exact=False): three receivers -- the synthetic FM stream, the weak stream with
    impulses at the block's ends and on both sides of tile seams and tiny_pattern planted in both calls, and silence -> constant -> random 0 / 255 -- two calls; each
    channel's demod tap against the model of the integer model's IF (tests/_fe_model.py; no IF tap in a bank), the sample in
    front of a block being the stream's (recomputed from the slot's history), zeros at the start."""
    T = 101
    p = fmrx.modeParams(mode, T, 101, 101)
    D, bb, calls = p.rf_decim, p.block_bytes, 2
    n = calls * bb // 2
    rng = np.random.default_rng(50 + mode)
    weak = weak_bytes(rng, 2 * n)
    spots = [0, bb // 2 - 1, bb // 2, n - 1] + [MFMA_SEAM * t * D + d for t in (1, 2, 17) for d in (-1, 0, 1)]
    spots += [bb // 2 + MFMA_SEAM * t * D + d for t in (1, 5) for d in (-1, 0, 1)] + [bb // 2 - 1 - (T - 1) // 2]
    for q in spots:
        weak[max(0, 2 * q - 8):2 * q + 10] = 128
    impulses(weak, sorted(set(spots)))
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, T)
    q = quantised_taps(h)
    pat = tiny_pattern(q)
    assert pat
    for k in (3 * MFMA_SEAM, 7 * MFMA_SEAM + 1, 20 * MFMA_SEAM + 59, bb // 2 // D + 2 * MFMA_SEAM, bb // 2 // D + 9 * MFMA_SEAM + 119):
        plant(weak, k * D, pat, q, T, D)
    third = np.full(2 * n, 128, U8)
    third[2 * (n // 4):2 * (n // 2):2], third[2 * (n // 4) + 1:2 * (n // 2):2] = 131, 120
    third[2 * (n // 2):] = rng.integers(0, 2, 2 * n - 2 * (n // 2)).astype(U8) * 255
    streams = [channel_stream(oracle, 0, n, p.rf_Fs), weak, third]
    ch = fmrx.Channels(mode, 3, rf_taps=T, audio_channels=audio_channels, exact=False)
    got = [[] for _ in streams]
    for k in range(calls):
        ch.process(np.stack([s[k * bb:(k + 1) * bb] for s in streams]), want_pcm=False)
        for c in range(3):
            got[c].append(ch.read_tap(c, "demod"))
    ch.close()
    for c, s in enumerate(streams):
        I, Q = fe.fe_model(s, np.full(2 * (T - 1), 128, U8), h, D)
        parts = check_demod(fmrx, np.concatenate(got[c]), I, Q, (0.0, 0.0), f"bank mode {mode} channel {c}")
        if c == 1:
            assert ((parts.den > 0) & (parts.den < dm.THRESHOLD)).sum() >= 5


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_mono_on_the_weak_stream(fmrx, oracle, mode):
    """mono_fused_kernel's discriminator never leaves the chip: its audio must equal the fma-chain model of the audio FIR
    (tests/_fir_model.py) fed the discriminator of the twin that keeps its intermediates -- which is pinned here to the model of
    the integer IF, on windows of the stream (all of the small blocks; the head, the tail and the middle of the big one).  A
    discriminator sample of the fused kernel that differed from the twin's by one bit would move the audio sums it enters.  Small
    blocks: general tiles; the big one has more batches than the largest grid has waves (two per wave): straight-line batches.
    Stream: weak, tiny_pattern planted every 3001 outputs, with random 0 / 255 stretches (silence -> full scale -> silence)."""
    p = fmrx.modeParams(mode)
    T, TA, D, DA = p.rf_taps, p.audio_taps, p.rf_decim, p.audio_decim
    unit = 2 * D * DA * 4
    cuts = [unit * 64, unit * 64 * 7 + unit, 2 * D * DA * 256 * 2200 + unit, 256 * unit]
    assert -(-cuts[2] // (2 * D * DA) // 256) > 2048
    rng = np.random.default_rng(60 + mode)
    stream = weak_bytes(rng, sum(cuts))
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, T)
    q = quantised_taps(h)
    pat = tiny_pattern(q)
    assert pat
    for n in range(300 * D, sum(cuts) // 2 - 2 * T, 3001 * D):
        plant(stream, n, pat, q, T, D)
    for a in (cuts[0] // 2, cuts[0] + cuts[1] + cuts[2] // 3, sum(cuts) - cuts[3] // 2):
        a = a // 16 * 16
        stream[a:a + 40 * D * 16] = rng.integers(0, 2, 40 * D * 16).astype(U8) * 255
    res = run_fused(fmrx, mode, T, TA, cut(stream, cuts), wraps=())
    x = check_fused(oracle, res, taps_of(fmrx, p)[2], T, D, TA, DA, f"fused mode {mode}, weak stream", False)
    assert x.any()
    # the twin's discriminator on windows [k0, k1) of IF outputs: the model of the integer model's IF
    n_if = len(x)
    edges = np.cumsum([0] + cuts) // (2 * D)
    wins = [(0, int(edges[2])), (int(edges[2]), int(edges[2]) + 40_000), (n_if // 2, n_if // 2 + 40_000),
            (int(edges[3]) - 40_000, n_if)]
    for k0, k1 in wins:
        lead = T - 1 + D                                     # bytes in front of the window: the taps' reach and output k0 - 1
        s0 = max(0, k0 * D - lead)
        hist = np.concatenate([np.full(2 * (T - 1), 128, U8), stream[2 * s0:2 * k0 * D]])
        I, Q = fe.fe_model(stream[2 * k0 * D:2 * k1 * D], hist, h, D, k0=-1 if k0 else 0)
        prev = (I[0], Q[0]) if k0 else (0.0, 0.0)
        I, Q = (I[1:], Q[1:]) if k0 else (I, Q)
        parts = check_demod(fmrx, x[k0:k1], I, Q, prev, f"fused mode {mode}: the twin's discriminator, outputs {k0}..{k1}")
        assert ((parts.den > 0) & (parts.den < dm.THRESHOLD)).any()
