"""The matrix-core front end (kernels_fe_mfma.hip: fe_mfma_kernel behind fmrx_fe_fir_decim_u8, fmrx_fe_run_dev and the
pipeline) checked BIT FOR BIT against the integer model of tests/_fe_model.py, at all nine (taps, decim) shapes of
FMRX_FE_MFMA_CASES, and the model itself against the float64 FIR within its stated bound.

What the looser oracle tests (tests/test_gpu_parity.py: 2e-6 relative RMS) cannot see and these pin down:
  * the ends of the tap window: impulseResponseLPF's h[0] is exactly 0 and h[1], h[T-1] are ~1e-5 of the peak, so
    here the taps are also random, end-heavy (|h[0]|, |h[T-1]| the largest), dyadic on rounding ties, of wide
    dynamic range, and at the ends of the accepted scale range;
  * every tap's position: single 0 / 255 bytes in silence at the block's ends, on both sides of every 120-output
    tile seam and inside the history (an impulse's response is the tap sequence itself);
  * full-scale and sign-aligned worst-case inputs, byte 0 (the one asymmetric int8 value) included;
  * the block sizes the kernel takes (multiples of 8 samples), from 8 samples to blocks where every wave runs the
    steady-state loop, and the history carried across blocks.
Every random-byte case also differs somewhere from force_generic=True: the matrix-core kernel ran (the plan's
`specialised` flag reports only the vector-ALU table)."""
import numpy as np
import pytest

import _fe_model as fm

pytestmark = pytest.mark.gpu

SHAPES = [(13, 10), (101, 10), (151, 10), (13, 5), (101, 5), (151, 5), (13, 3), (101, 3), (151, 3)]   # FMRX_FE_MFMA_CASES
VALU_SHAPES = list(SHAPES)                                                                            # FMRX_FE_CASES
RF_FS = {10: 2.4e6, 5: 1.44e6, 3: 960e3}
U8 = np.uint8


@pytest.fixture(autouse=True)
def mfma_variant(fmrx):
    """Every test here starts on the matrix-core variant (the default) and leaves the option as it found it."""
    old = fmrx.get_option("fe_variant")
    fmrx.set_option("fe_variant", "mfma")
    try:
        yield
    finally:
        fmrx.set_option("fe_variant", old)


def silence(T):
    return np.full(2 * (T - 1), 128, U8)


def run(fmrx, iq, h, D, hist=None, msg="", differs=True):
    """frontEndFIR on the default (matrix-core) path, checked against the model; differs: also against the generic
    kernel, which must disagree somewhere (random bytes: the float32 sum of the unquantised taps is another number)."""
    T = len(h)
    fi, fq, _ = fmrx.frontEndFIR(iq, h, D, hist)
    want = fm.fe_check(iq, silence(T) if hist is None else hist, h, D, fi, fq, msg=msg)
    if differs:
        gi, gq, _ = fmrx.frontEndFIR(iq, h, D, hist, force_generic=True)
        assert (gi.view(np.uint32) != fi.view(np.uint32)).any() or (gq.view(np.uint32) != fq.view(np.uint32)).any(), \
            (msg, "output equals the generic kernel's: the matrix-core kernel did not run")
    return want


def tapset(fmrx, kind, T, D, rng):
    if kind == "lpf":
        return fmrx.impulseResponseLPF(RF_FS[D], 100e3, T)
    if kind == "random":
        return (rng.standard_normal(T) * 0.05).astype(np.float32)
    if kind == "end_heavy":                               # the ends of the window carry the largest taps, opposite signs
        h = (rng.standard_normal(T) * 0.02).astype(np.float32)
        h = np.clip(h, -0.2, 0.2)
        h[0], h[-1] = 0.3, -0.29
        return h.astype(np.float32)
    if kind == "dyadic_ties":                             # h * 2^22 on exact half-integers: llround rounds away from 0
        m = rng.integers(0, 1 << 21, T) + 0.5
        h = np.ldexp(m * rng.choice([-1.0, 1.0], T), -22)
        h[T // 2] = 1.0                                   # max|h| = 1 -> s = 22
        h[0], h[-1] = -np.ldexp(2.5, -22), np.ldexp(0.5, -22)
        return h.astype(np.float32)
    if kind == "wide_range":                              # 2^-40 .. 1: the small taps quantise to 0 / +-1
        h = np.ldexp(rng.choice([-1.0, 1.0], T), -rng.integers(0, 41, T)).astype(np.float32)
        h[T // 3] = 1.0
        h[0], h[-1] = np.ldexp(1.0, -23), -np.ldexp(1.0, -23)   # exactly 0.5 and -0.5 after scaling: +1 and -1
        if T > 4:
            h[1], h[-2] = np.ldexp(1.0, -24), -np.ldexp(3.0, -24)
        return h
    if kind.startswith("max_"):                           # scale extremes: max|h| as given (float32)
        v = np.float32(float(kind[4:]))
        h = rng.standard_normal(T)
        h = (h / np.max(np.abs(h)) * np.float64(v)).astype(np.float32)
        h[0] = -v
        return h
    raise ValueError(kind)


BELOW_1E30 = float(np.nextafter(np.float32(1e30), np.float32(0)))   # float32(1e30) itself is > 1e30: rejected
KINDS = ["lpf", "random", "end_heavy", "dyadic_ties", "wide_range",
         "max_1.0000001e-30", "max_5e-30", "max_1e-29", "max_1e29", f"max_{BELOW_1E30!r}"]


def sign_aligned(h, D, n, rng):
    """Uniform bytes, overwritten every few outputs with a window whose I samples carry the signs of the taps at full
    scale (127 / -128) and whose Q samples carry the opposite polarity: the largest |acc| the taps allow."""
    T = len(h)
    pos = np.where(h >= 0, 127, -128)[::-1] + 128         # oldest sample first
    iq = rng.integers(0, 256, 2 * n, dtype=U8)
    step = D * (-(-T // D) + 1)
    for p in range(D * (-(-(T - 1) // D)), n, step):
        iq[2 * (p - T + 1):2 * (p + 1):2] = pos
        iq[2 * (p - T + 1) + 1:2 * (p + 1):2] = 255 - pos
    return iq


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,D", SHAPES)
def test_taps_bit_exact(fmrx, T, D, kind):
    """Each kind of tap set, uniform full-scale bytes with a random history and sign-aligned worst-case windows:
    bit-equal to the integer model.  The block (4 tiles and a ragged fifth) is not a multiple of D."""
    rng = np.random.default_rng(T * 1000 + D * 10 + KINDS.index(kind))
    h = tapset(fmrx, kind, T, D, rng)
    assert fm.fe_scale(h) is not None, kind
    if kind == "dyadic_ties":
        assert fm.fe_scale(h) == 22
    if kind == "max_1.0000001e-30":
        assert fm.scales(fm.fe_scale(h))[0] < np.finfo(np.float32).tiny   # scale_lo is a float32 subnormal
    n = 480 * D + 8 * D + 8
    iq = rng.integers(0, 256, 2 * n, dtype=U8)
    hist = rng.integers(0, 256, 2 * (T - 1), dtype=U8)
    run(fmrx, iq, h, D, hist, msg=f"{kind} uniform")
    run(fmrx, sign_aligned(h, D, n, rng), h, D, hist, msg=f"{kind} sign-aligned")


@pytest.mark.parametrize("T,D", SHAPES)
def test_rejected_taps_take_the_generic_kernel(fmrx, oracle, T, D):
    """Tap sets fe_mfma_scale rejects (non-finite, all zero, max|h| out of [1e-30, 1e30]) run the generic kernel: bit-equal
    to the oracle's convolveBlockFastFIR; where the oracle gives NaN both sides are NaN.  All-zero taps (h[0] == 0) take
    the vector-ALU kernel instead: exact zeros."""
    rng = np.random.default_rng(T + 7 * D)
    n = 480 * D + 16
    iq = rng.integers(0, 256, 2 * n, dtype=U8)
    hist = rng.integers(0, 256, 2 * (T - 1), dtype=U8)
    f = oracle.u8_to_f32(iq)
    fh = oracle.u8_to_f32(hist)
    base = (rng.standard_normal(T) * 0.05).astype(np.float32)
    cases = {"zero": np.zeros(T, np.float32)}
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        h = base.copy()
        h[T // 2] = bad
        cases[name] = h
    for name, v in (("max_5e-31", 5e-31), ("max_2e30", 2e30), ("max_f32(1e30)", 1e30)):
        h = (base / np.max(np.abs(base)) * np.float64(np.float32(v))).astype(np.float32)
        h[0] = np.float32(v)
        cases[name] = h
    for name, h in cases.items():
        assert fm.fe_scale(h) is None, name
        fi, fq, _ = fmrx.frontEndFIR(iq, h, D, hist)
        for got, c in ((fi, 0), (fq, 1)):
            want, _ = oracle.convolve_block_fast_fir(f[c::2], h, fh[c::2].copy(), D)
            if name == "zero":
                assert not got.any() and not want.any(), name
                continue
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (name, "NaN positions differ")
            assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), name


def impulse_blocks(T, D, n):
    """(name, block, history) with one 0 byte on one channel and one 255 byte on the other at the same sample, in silence:
    the block's first and last sample, both sides of every tile seam (120 outputs = 120*D samples), the history."""
    spots = [("block", 0), ("block", n - 1)]
    for t in range(1, -(-(n // D) // 120)):
        spots += [("block", 120 * t * D + d) for d in (-1, 0, 1)]
    spots += [("hist", 0), ("hist", (T - 1) // 2), ("hist", T - 2)]
    for where, p in spots:
        for ci in (0, 1):
            iq, hist = np.full(2 * n, 128, U8), silence(T)
            buf = iq if where == "block" else hist
            buf[2 * p + ci], buf[2 * p + 1 - ci] = 0, 255
            yield f"{where} sample {p}, byte 0 on {'IQ'[ci]}", iq, hist


@pytest.mark.parametrize("kind", ["end_heavy", "lpf"])
@pytest.mark.parametrize("T,D", SHAPES)
def test_inputs_bit_exact(fmrx, T, D, kind):
    """Constant blocks 0, 255, 128 (the last: exact zeros), and single impulses on the block's ends, the tile seams and
    the history: bit-equal to the model.  An impulse's response is the tap sequence, so these pin every tap's position;
    with end-heavy taps a dropped or shifted h[0] / h[T-1] is off by ~0.3/128, not by 1e-5 of the peak."""
    rng = np.random.default_rng(3 * T + D)
    h = tapset(fmrx, kind, T, D, rng)
    n = 480 * D
    for u in (0, 255, 128):
        want = run(fmrx, np.full(2 * n, u, U8), h, D, np.full(2 * (T - 1), u, U8), msg=f"constant {u}", differs=False)
        if u == 128:
            assert not want[0].any() and not want[1].any()
    for name, iq, hist in impulse_blocks(T, D, n):
        run(fmrx, iq, h, D, hist, msg=name, differs=False)


@pytest.mark.parametrize("T,D", SHAPES)
def test_smallest_block(fmrx, T, D):
    """n = 8 samples, the smallest block the matrix-core kernel takes (no history given: silence in front)."""
    rng = np.random.default_rng(T * D)
    h = tapset(fmrx, "end_heavy", T, D, rng)
    iq = rng.integers(0, 256, 16, dtype=U8)
    run(fmrx, iq, h, D, None, msg="n = 8", differs=False)   # 0 to 2 outputs: they may all agree with the generic kernel


@pytest.mark.parametrize("T,D", [(151, 10), (101, 5), (13, 3)])
def test_output_count_sweep(fmrx, T, D):
    """Every block size of 8k samples up to 241 outputs (the matrix-core path needs 2n % 16 == 0; for D = 10 that is every
    output count 0..241): ragged tiles, n not a multiple of D, a single partial tile.  From 16 outputs up, each block
    also differs from the generic kernel somewhere (fewer outputs may all agree with it by chance)."""
    rng = np.random.default_rng(T + D + 5)
    h = tapset(fmrx, "end_heavy", T, D, rng)
    iq = rng.integers(0, 256, 2 * 242 * D + 16, dtype=U8)
    seen = set()
    for n in range(8, 242 * D + 8, 8):
        if n // D > 241:
            break
        seen.add(n // D)
        run(fmrx, iq[:2 * n], h, D, None, msg=f"n = {n}", differs=n // D >= 16)
    assert min(seen) == 8 // D and max(seen) >= 241 - D


def mf_cfg(T, D):
    """MfCfg / launch_mfma / fe_mfma_launch's formulas: (P, resident waves of the grid)."""
    col = 2 * D * 8
    front = (2 * (T - 1) + 15) // 16 * 16
    ksteps = (front + 2 * D * 7 + 2 + 63) // 64
    tile_win = col * 15 + 64 * ksteps
    slot = -(-tile_win // 1024) * 1024
    small = T <= 101
    minb = 3 if small and D == 3 else 4 if small and D == 5 else 2
    pf = 4 if small and D == 3 else 2 if small and D == 5 else 0
    P = pf or min(max(8192 // tile_win, 2), 8)
    wgs = min(160 * 1024 // (4 * (P + 1) * slot), minb)
    return P, 4 * 256 * wgs


@pytest.mark.parametrize("T,D", [(151, 10), (13, 5), (101, 3)])
def test_steady_state_block(fmrx, T, D):
    """One block per D in which every wave of the full grid runs 3P + 4 >= 2(P+1) tiles: past its ramp-up, so that the
    straight-line loop (fast_loop, D < 10) and the steady counted waits run on most tiles."""
    P, waves = mf_cfg(T, D)
    n_tiles = (3 * P + 4) * waves
    n = n_tiles * 120 * D
    rng = np.random.default_rng(T * D + 99)
    h = tapset(fmrx, "end_heavy", T, D, rng)
    iq = rng.integers(0, 256, 2 * n, dtype=U8)
    hist = rng.integers(0, 256, 2 * (T - 1), dtype=U8)
    run(fmrx, iq, h, D, hist, msg=f"{n_tiles} tiles")


@pytest.mark.parametrize("T,D", SHAPES)
def test_stream_with_history(fmrx, T, D):
    """Four consecutive blocks through the host API with its history carried: the concatenation equals the model of the
    whole stream (block sizes are multiples of D, so the outputs sit where the stream's do)."""
    rng = np.random.default_rng(T * 7 + D)
    h = tapset(fmrx, "end_heavy", T, D, rng)
    L = int(np.lcm(8, D))
    sizes = [L * max(k, -(-(T - 1) // L)) for k in (37, 1, 64, 19)]
    stream = rng.integers(0, 256, 2 * sum(sizes), dtype=U8)
    hist, off, got_i, got_q = silence(T), 0, [], []
    for nb in sizes:
        blk = stream[2 * off:2 * (off + nb)]
        fi, fq, hist = fmrx.frontEndFIR(blk, h, D, hist)
        assert np.array_equal(hist, blk[-2 * (T - 1):])
        got_i.append(fi)
        got_q.append(fq)
        off += nb
    fm.fe_check(stream, silence(T), h, D, np.concatenate(got_i), np.concatenate(got_q), msg="stream")


@pytest.mark.parametrize("T,D", SHAPES)
def test_run_dev_history_prefix_is_dead(fmrx, T, D):
    """FrontEndPlan.run_dev with a device history of history_bytes: random bytes in front of the live 2(T-1) do not reach
    the IF outputs (two different prefixes, the same outputs, equal to the model of the live bytes)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(T * 11 + D)
    h = tapset(fmrx, "end_heavy", T, D, rng)
    plan = fmrx.FrontEndPlan(h, D)
    hb = plan.history_bytes
    assert hb % 16 == 0 and hb >= 2 * (T - 1)
    n = 480 * D + 40
    iq = rng.integers(0, 256, 2 * n, dtype=U8)
    live = rng.integers(0, 256, 2 * (T - 1), dtype=U8)
    d_iq = torch.from_numpy(iq).cuda()
    outs = []
    for _ in range(2):
        buf = np.concatenate([rng.integers(0, 256, hb - len(live), dtype=U8), live])
        d_hist = torch.from_numpy(buf).cuda()
        d_if = torch.zeros(2 * (n // D), dtype=torch.float32, device="cuda")
        plan.run_dev(d_iq.data_ptr(), n, d_hist.data_ptr(), d_if.data_ptr())
        torch.cuda.synchronize()
        outs.append(d_if.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    fm.fe_check(iq, live, h, D, outs[0][0::2], outs[0][1::2], msg="run_dev")
    plan.close()


@pytest.mark.parametrize("T,D", VALU_SHAPES)
def test_vector_alu_kernel(fmrx, oracle, T, D):
    """fe_variant valu: taps with h[0] == 0 run the vector-ALU kernel (specialised), within gamma_T sum|h_k||x_k|/128 of the
    float64 FIR, gamma_T = T u / (1 - T u), u = 2^-24 (one fma per tap on exact products h/128 * x); taps with h[0] != 0
    fall back to the generic kernel: bit-equal to the oracle."""
    fmrx.set_option("fe_variant", "valu")
    try:
        rng = np.random.default_rng(T * 13 + D)
        n = 480 * D + 8
        iq = rng.integers(0, 256, 2 * n, dtype=U8)
        hist = rng.integers(0, 256, 2 * (T - 1), dtype=U8)
        u = 2.0 ** -24
        gamma = T * u / (1 - T * u)
        r = (rng.standard_normal(T) * 0.05).astype(np.float32)
        r[0] = 0.0
        for h in (tapset(fmrx, "lpf", T, D, rng), r):
            assert fmrx.FrontEndPlan(h, D).specialised
            fi, fq, _ = fmrx.frontEndFIR(iq, h, D, hist)
            h64 = h.astype(np.float64)
            for c, got in enumerate((fi, fq)):
                f64, bnd = [], []
                for _, w in fm.windows(iq, hist, T, D, c):
                    f64.append(w @ h64 / 128)
                    bnd.append(gamma * (np.abs(w) @ np.abs(h64)) / 128)
                err = np.abs(got.astype(np.float64) - np.concatenate(f64))
                assert np.all(err <= np.concatenate(bnd)), ("IQ"[c], float(np.max(err - np.concatenate(bnd))))
        h = r.copy()
        h[0] = 0.01
        assert not fmrx.FrontEndPlan(h, D).specialised
        fi, fq, _ = fmrx.frontEndFIR(iq, h, D, hist)
        f, fh = oracle.u8_to_f32(iq), oracle.u8_to_f32(hist)
        for c, got in enumerate((fi, fq)):
            want, _ = oracle.convolve_block_fast_fir(f[c::2], h, fh[c::2].copy(), D)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "IQ"[c]
    finally:
        fmrx.set_option("fe_variant", "mfma")


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline's front end: IF stream and discriminator
# ---------------------------------------------------------------------------------------------------------------------
C1 = 2.0 + 2.0 ** -16
C2 = 6.0 + 2.0 ** -16


def assert_demod(got, i, q, pi, pq, msg):
    """demod_fast / demod_fast_bounded against the float64 discriminator of the same float32 IF values.

    The kernels compute num = RN(RN(i RN(q-pq)) - RN(q RN(i-pi))), den = RN(RN(i i) + RN(q q)) and RN(num * rcp(den)),
    rcp = v_rcp_f32 within 1 ulp (relative 2u, u = 2^-24); the 2^64 pre-scaling of demod_fast is exact.  With
    a = i(q-pq), b = q(i-pi) (exact), d = (a-b)/den (exact):
      RN(i RN(q-pq)) = a(1+alpha), |alpha| <= gamma_2 = 2u/(1-2u), the same for b, so
      num = (a - b + a alpha - b beta)(1+eps);  den' = den(1+theta), |theta| <= gamma_2;
      result = (d + (a alpha - b beta)/den) (1+eps)(1+rho)(1+eta)/(1+theta), |rho| <= 2u, |eps|, |eta| <= u,
    hence |result - d| <= gamma_2 (1+phi) (|a|+|b|)/den + phi |d|, phi = 6u + O(u^2):
      c1 u (|i||q-pq| + |q||i-pi|)/den + c2 u |d|,  c1 = 2 + 2^-16, c2 = 6 + 2^-16 (the slack covers the O(u^2) terms).
    Where den == 0 the result is exactly 0."""
    u = 2.0 ** -24
    d, ab, den = fm.discriminator_f64(i, q, pi, pq)
    got = np.asarray(got, np.float32)
    assert got.shape == d.shape, (msg, got.shape, d.shape)
    z = den == 0
    assert not got[z].view(np.uint32).any(), (msg, "den == 0 must give exactly +0")
    nz = ~z
    bnd = C1 * u * ab[nz] / den[nz] + C2 * u * np.abs(d[nz])
    err = np.abs(got[nz].astype(np.float64) - d[nz])
    assert np.all(err <= bnd), (msg, int(np.sum(err > bnd)), float(np.max(err / bnd)))


def pipeline_stream(rng, sizes, n_silent):
    """Uniform full-scale bytes, then low-amplitude bytes (127..129: den tiny), then a silent stretch, then uniform."""
    n = sum(sizes)
    s = rng.integers(0, 256, n, dtype=U8)
    a, b = n // 4, n // 2
    s[a:b] = rng.integers(127, 130, b - a, dtype=U8)
    s[b:b + n_silent] = 128
    return s


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rf_taps", [13, 101, 151])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_pipeline_front_end(fmrx, oracle, mode, rf_taps, channels):
    """The pipeline's matrix-core front end (designed taps, keep_intermediates on): if_i / if_q bit-equal to the model of
    the whole stream, demod within the bound of assert_demod of the float64 discriminator on those IF values (the first
    output of each block takes its previous sample from the last block), exactly 0 where den == 0.  Then mode 3 with
    keep_intermediates off (the demod-only instantiation)."""
    p = oracle.mode_params(mode, rf_taps, 101, 101)
    D, A, U = p.rf_decim, p.audio_decim, max(p.audio_upsamp, 1)
    step = np.lcm(A // np.gcd(A, U), 8)
    unit = int(2 * D * step)
    floor = -(-max(2 * (rf_taps - 1), 2 * D * 128) // unit) * unit
    sizes = [max(unit * k, floor) for k in ((13, 1, 57, 2, 7) if U == 1 else (1, 3, 1, 2))]
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, rf_taps)
    rng = np.random.default_rng(mode * 1000 + rf_taps * 2 + channels)
    stream = pipeline_stream(rng, sizes, 2 * D * (rf_taps + 64))
    hist0 = silence(rf_taps)
    want_i, want_q = fm.fe_model(stream, hist0, h, D)
    for keep in ((True, False) if mode == 3 else (True,)):
        pl = fmrx.Pipeline(mode, channels, rf_taps=rf_taps, max_block_bytes=max(sizes))
        pl.set_option("fe_variant", "mfma")
        pl.set_keep_intermediates(keep)
        off = 0
        for nb in sizes:
            pl.process(stream[off:off + nb], want_pcm=False)
            k0, k1 = off // (2 * D), (off + nb) // (2 * D)
            i, q = want_i[k0:k1], want_q[k0:k1]
            pi = np.concatenate([want_i[k0 - 1:k0] if k0 else [0.0], i[:-1]])
            pq = np.concatenate([want_q[k0 - 1:k0] if k0 else [0.0], q[:-1]])
            msg = f"mode {mode} taps {rf_taps} ch {channels} keep {keep} block at byte {off}"
            if keep:
                gi, gq = pl.read_tap("if_i"), pl.read_tap("if_q")
                for got, want, c in ((gi, i, "I"), (gq, q, "Q")):
                    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                    assert bad.size == 0, (msg, c, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
            assert_demod(pl.read_tap("demod"), i, q, pi, pq, msg)
            off += nb
        assert off == len(stream)
        pl.close()
    # the model itself against the float64 FIR on this stream
    fm.fe_check(stream, hist0, h, D, want_i, want_q, msg="model")


@pytest.mark.parametrize("mode", [1, 3])
def test_pipeline_steady_state_block(fmrx, oracle, mode):
    """One pipeline block big enough that every wave of the full grid runs 3P + 4 tiles: the straight-line loop with the
    discriminator (demod_fast_bounded; D < 10) in both of its forms, IF + demod (keep_intermediates on) and demod only
    (off, mode 3; mode 1 mono without the IF stream takes the fused audio kernel instead)."""
    p = oracle.mode_params(mode, 101, 101, 101)
    D, A, U = p.rf_decim, p.audio_decim, max(p.audio_upsamp, 1)
    unit = int(2 * D * np.lcm(A // np.gcd(A, U), 8))
    P, waves = mf_cfg(101, D)
    nb = -(-2 * (3 * P + 4) * waves * 120 * D // unit) * unit
    h = fmrx.impulseResponseLPF(p.rf_Fs, 100e3, 101)
    rng = np.random.default_rng(mode + 404)
    blk = rng.integers(0, 256, nb, dtype=U8)
    want_i, want_q = fm.fe_model(blk, silence(101), h, D)
    pi, pq = np.concatenate([[0.0], want_i[:-1]]), np.concatenate([[0.0], want_q[:-1]])
    for keep in ((True, False) if mode == 3 else (True,)):
        pl = fmrx.Pipeline(mode, 1, max_block_bytes=nb)
        pl.set_option("fe_variant", "mfma")
        pl.set_keep_intermediates(keep)
        pl.process(blk, want_pcm=False)
        msg = f"mode {mode} keep {keep} {nb} bytes"
        if keep:
            for k, want in (("if_i", want_i), ("if_q", want_q)):
                got = pl.read_tap(k)
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, (msg, k, bad.size, bad[:8].tolist())
        assert_demod(pl.read_tap("demod"), want_i, want_q, pi, pq, msg)
        pl.close()
