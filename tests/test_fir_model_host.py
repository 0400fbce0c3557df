"""The fma-chain model of the packed-FMA FIR kernels (tests/_fir_model.py) against exact rational arithmetic, the float64
FIR, and the reference's order; and the shape lists tests/test_gpu_fir_exact.py covers.  No GPU involved."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _fir_model as fm
from test_fe_model_host import parse_cases, rn_f32

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "software-defined-radio_amd", "csrc")
F32 = np.float32


def exact_fma(a, b, c):
    """RN32(a b + c) on rationals; the sign of an exact zero by IEEE 754's rule (round to nearest)."""
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if r == 0:
        # -0 only for (-0 product) + (-0); an exact cancellation of non-zero terms is +0
        p_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        if (a == 0 or b == 0) and c == 0 and p_neg and np.signbit(c):
            return F32(-0.0)
        return F32(0.0)
    return rn_f32(r)


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def check_fma(a, b, c):
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    got = fm.fmaf(a, b, c)
    want = np.array([exact_fma(x, y, z) for x, y, z in zip(a, b, c)], F32)
    np.testing.assert_array_equal(bits(got), bits(want))
    return want


def test_fmaf_random_triples():
    rng = np.random.default_rng(11)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 60, n)).astype(F32)
    # half of them with c near -a b: cancellation down to a few bits
    c[::2] = (-(a[::2].astype(np.float64) * b[::2]) * (1 + rng.standard_normal(n // 2) * 2.0 ** -20)).astype(F32)
    check_fma(a, b, c)


def double_rounding_triples():
    """a b + c lands, in float64, exactly on a float32 midpoint that the exact value misses by 2^-70 relative; the tie
    then goes to the even neighbour, the wrong one."""
    one_p = F32(1 + 2.0 ** -23)
    one_m = F32(1 - 2.0 ** -23)                       # (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46
    out = []
    for k in (-100, -20, 0, 20, 100):
        s = 2.0 ** k
        # exact = c + 2^-24 s - 2^-70 s, just below the midpoint above the odd c: the answer is c, ties-to-even gives c + ulp
        out.append((one_p, F32(one_m * 2.0 ** -24 * s), F32((1 + 2.0 ** -23) * s)))
        # exact = c - 2^-24 s + 2^-70 s, just above the midpoint below the odd c: the answer is c, ties-to-even gives c - ulp
        out.append((-one_p, F32(one_m * 2.0 ** -24 * s), F32((1 + 2.0 ** -22 + 2.0 ** -23) * s)))
    out += [(-a, b, -c) for a, b, c in out]
    return [tuple(F32(v) for v in t) for t in out]


def test_fmaf_double_rounding_cases():
    t = double_rounding_triples()
    a, b, c = (np.array(v, F32) for v in zip(*t))
    want = check_fma(a, b, c)
    plain = fm.fmaf_via_f64(a, b, c)
    assert (bits(plain) != bits(want)).all(), "the plain float64 route must get every constructed case wrong"
    assert (want == c).all()


def test_fmaf_subnormal_zero_and_cancellation():
    tiny = F32(np.ldexp(1.0, -149))
    rng = np.random.default_rng(5)
    a = (rng.uniform(1, 2, 500) * 2.0 ** -70).astype(F32)
    b = (rng.uniform(-2, 2, 500) * 2.0 ** -70).astype(F32)
    c = (rng.integers(-3000, 3000, 500) * tiny).astype(F32)      # subnormal addends, results subnormal
    w = check_fma(a, b, c)
    assert (np.abs(w) < np.finfo(F32).tiny).sum() > 400
    z = F32(0.0)
    cases = [(z, F32(1), z), (F32(-0.0), F32(1), F32(-0.0)), (F32(-0.0), F32(1), z), (z, F32(-1), F32(-0.0)),
             (F32(-0.0), F32(-0.0), F32(-0.0)), (F32(1), F32(1), F32(-1)), (F32(3), F32(-5), F32(15)),
             (F32(-1.5), F32(2.0 ** -20), F32(1.5 * 2.0 ** -20)), (tiny, F32(0.5), z), (tiny, F32(0.5), tiny),
             (tiny, F32(1.5), z), (tiny, F32(-0.5), F32(-0.0)), (F32(2.0 ** -75), F32(2.0 ** -75), z)]
    a, b, c = (np.array(v, F32) for v in zip(*cases))
    w = check_fma(a, b, c)
    assert bits(w[:5]).tolist() == [0, 0x80000000, 0, 0x80000000, 0]
    assert (w[5:8] == 0).all() and not np.signbit(w[5:8]).any()   # exact cancellation: +0
    assert w[8] == 0 and w[9] == 2 * tiny and w[10] == 2 * tiny and w[12] == 0   # ties to even at 2^-150


def scalar_chain(x, h, order, D, delay, k):
    acc = F32(0.0)
    for n in order:
        i = D * k - n - delay
        xv = x[i] if i >= 0 else F32(0.0)
        acc = exact_fma(xv, h[n], acc)
    return acc


@pytest.mark.parametrize("kind", ["ascending", "descending", "polyphase"])
def test_chain_equals_sequential_exact_fma(kind):
    rng = np.random.default_rng({"ascending": 1, "descending": 2, "polyphase": 3}[kind])
    for T, D, delay in [(7, 1, 0), (13, 5, 6), (9, 3, 4), (13, 6, 0), (5, 2, 1)]:
        order = {"ascending": fm.ascending(T), "descending": fm.descending(T), "polyphase": fm.polyphase(T, D)}[kind]
        assert sorted(order) == list(range(T))
        x = (rng.standard_normal(6 * D + 11) * 2.0 ** rng.integers(-8, 8)).astype(F32)
        h = rng.standard_normal(T).astype(F32)
        k0 = 2
        y = fm.fma_chain(x, h, order, D, delay, k0=k0, n_out=len(x) // D - k0)
        want = np.array([scalar_chain(x, h, order, D, delay, k0 + j) for j in range(len(y))], F32)
        np.testing.assert_array_equal(bits(y), bits(want), err_msg=f"{kind} T={T} D={D}")


def test_polyphase_order_is_au_step():
    """audio_fir_kernel: table entry p*NC*12 + q holds h[T-1-m], m = p + D q; au_step walks p, then q ascending."""
    assert fm.polyphase(13, 5) == [12, 7, 2, 11, 6, 1, 10, 5, 0, 9, 4, 8, 3]
    for T, D in [(101, 5), (101, 6), (13, 6)]:
        o = fm.polyphase(T, D)
        assert sorted(o) == list(range(T)) and o[0] == T - 1


def demod_stream(oracle, mode, nblk=3):
    p = oracle.mode_params(mode)
    iq = oracle.synth_fm_u8(p.block_bytes // 2 * nblk, rf_Fs=p.rf_Fs)
    return np.concatenate([oracle.pipeline(mode, 2).process(iq[b * p.block_bytes:(b + 1) * p.block_bytes])["demod"]
                           for b in range(nblk)]), p


def production_taps(oracle, fs, T):
    return {"lpf": oracle.impulse_response_lpf(fs, 16e3, T), "bpf_st": oracle.band_pass(fs, 22e3, 54e3, T),
            "bpf_car": oracle.band_pass(fs, 18.5e3, 19.5e3, T)}


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_chain_within_gamma_bound_of_float64(oracle, mode):
    """Every order of T fmas is within gamma_T sum|h x| of the float64 FIR, on the production taps at the mode's IF rate
    and a synthetic discriminator stream."""
    x, p = demod_stream(oracle, mode)
    for T in (13, 101, 151):
        for name, h in production_taps(oracle, float(p.if_Fs), T).items():
            for D, delay in ((1, 0), (5, (T - 1) // 2), (6, 0)):
                y64, a = fm.fir64(x, h, D, delay)
                for order in (fm.ascending(T), fm.descending(T), fm.polyphase(T, D)):
                    y = fm.fma_chain(x, h, order, D, delay)
                    err = np.abs(y.astype(np.float64) - y64)
                    assert (err <= fm.gamma(T) * a).all(), (mode, T, name, D)


@pytest.mark.parametrize("mode", [0, 1])
def test_fma_chain_differs_from_reference_order(oracle, mode):
    """ref_chain is the oracle's convolve_block_fir / convolve_block_fast_fir bit for bit (the reference's order), and on
    the discriminator stream the fma chain differs from it somewhere in every order: a GPU test that requires the chain
    cannot pass on a kernel that kept the reference's order (the generic fallback)."""
    x, p = demod_stream(oracle, mode)
    n_if = len(x) // 3
    D = p.audio_decim
    for T in (13, 101, 151):
        taps = production_taps(oracle, float(p.if_Fs), T)
        st = np.zeros(T - 1, F32)
        got, ref = [], fm.ref_chain(x, taps["bpf_st"])
        for b in range(3):
            y, st = oracle.convolve_block_fir(x[b * n_if:(b + 1) * n_if], taps["bpf_st"], st)
            got.append(y)
        np.testing.assert_array_equal(bits(np.concatenate(got)), bits(ref))
        st, got = np.zeros(T - 1, F32), []
        ref_d = fm.ref_chain(x, taps["lpf"], D)
        for b in range(3):
            y, st = oracle.convolve_block_fast_fir(x[b * n_if:(b + 1) * n_if], taps["lpf"], st, D)
            got.append(y)
        np.testing.assert_array_equal(bits(np.concatenate(got)), bits(ref_d))
        for order in (fm.ascending(T), fm.descending(T)):
            assert (bits(fm.fma_chain(x, taps["bpf_st"], order)) != bits(ref)).any()
            assert (bits(fm.fma_chain(x, taps["bpf_car"], order)) != bits(fm.ref_chain(x, taps["bpf_car"]))).any()
            assert (bits(fm.fma_chain(x, taps["lpf"], order, D)) != bits(ref_d)).any()
        assert (bits(fm.fma_chain(x, taps["lpf"], fm.polyphase(T, D), D)) != bits(ref_d)).any()
        # and ascending and descending chains differ from each other: the GPU test tells the two orders apart
        assert (bits(fm.fma_chain(x, taps["bpf_st"], fm.ascending(T))) != bits(fm.fma_chain(x, taps["bpf_st"], fm.descending(T)))).any()


@pytest.mark.parametrize("mode", [0, 1])
def test_fused_audio_row_phase(oracle, mode):
    """fused_audio(row0=r): the rows the fused mono bank gives a channel whose first kept output is not at a multiple of
    16 in the launch.  row0 = 0 is the model of the single-stream pipeline, unchanged; r = 4, 8, 12 equal the block that
    starts r outputs earlier with those outputs dropped (also at the start of the stream, where there is no earlier
    output), stay within gamma(4 AK + 1) sum|h x| of the float64 FIR, and differ in bits from row0 = 0 -- except
    where the rows' windows lie a whole number of MFMA groups apart (16 samples: DA r a multiple of 16, which is r = 8 at
    DA = 6): every tap then keeps its chain and its place in it, and the bits are those of row0 = 0."""
    x, p = demod_stream(oracle, mode)
    DA = p.audio_decim
    n_all = len(x) // DA
    for TA in (101, 13):
        h = oracle.impulse_response_lpf(float(p.if_Fs), 16e3, TA)
        y0 = fm.fused_audio(x, h, DA)
        np.testing.assert_array_equal(bits(fm.fused_audio(x, h, DA, row0=0)), bits(y0))
        np.testing.assert_array_equal(bits(fm.fused_audio(x, h, DA, 1024, 1024, row0=0)), bits(fm.fused_audio(x, h, DA, 1024, 1024)))
        y64, a = fm.fir64(x, h, DA)
        bound = fm.gamma(4 * fm.audio_mfma_ksteps(TA, DA) + 1) * a
        for r in (4, 8, 12):
            y = fm.fused_audio(x, h, DA, row0=r)
            assert len(y) == n_all
            assert (np.abs(y.astype(np.float64) - y64) <= bound).all(), (mode, TA, r)
            assert fm.row_phase_changes_bits(DA, r) == bool((bits(y) != bits(y0)).any()), (mode, TA, r)
            # a later block: the same as starting r outputs earlier
            k0, n = 1024 + 28, 1024
            np.testing.assert_array_equal(bits(fm.fused_audio(x, h, DA, k0, n, row0=r)), bits(fm.fused_audio(x, h, DA, k0 - r, n + r)[r:]))
            assert fm.row_phase_changes_bits(DA, r) == bool((bits(fm.fused_audio(x, h, DA, k0, n, row0=r)) != bits(fm.fused_audio(x, h, DA, k0, n))).any())
    assert [r for r in (0, 4, 8, 12) if fm.row_phase_changes_bits(DA, r)] == {5: [4, 8, 12], 6: [4, 12]}[DA]


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("mode", [0, 1])
def test_mono_tolerance_is_blind_to_seam_and_phase_errors(oracle, mode):
    """What the mono tolerance (RMS 2e-6 over a block) cannot see and the bit comparison of
    tests/test_gpu_mono_banks_exact.py can, on one 1024-output block of a bank channel (row phase 4, production taps):
      a. the oldest sample the block reads -- the first one in front of the filter's reach into the history -- is a
         neighbour's full-scale discriminator value (a history one sample short, a junk count off by one);
      b. the row phase is wrong by 4 (the outputs landed on other rows of the launch than the model's);
      c. one history sample at the far end of the filter's reach is zero (a history byte not moved).
    Each differs from the model in bits and stays below 2e-6 RMS: h[TA-1] is about 5e-5 of the peak tap, and a row phase
    only regroups the rounding.  For contrast, the sample directly in front of the block meets every fifth (sixth) tap:
    that one the tolerance does see."""
    x, p = demod_stream(oracle, mode)
    DA, TA = p.audio_decim, 101
    h = oracle.impulse_response_lpf(float(p.if_Fs), 16e3, TA)
    k0, n, row = 1024, 1024, 4
    y = fm.fused_audio(x, h, DA, k0, n, row0=row)
    full_scale = F32(np.pi)                                  # the discriminator's range: |x| <= pi (times a gain below 1)
    assert np.abs(x).max() <= full_scale
    far = DA * k0 - (TA - 1)                                 # x[DA k0 - n], n = TA-1: the oldest sample output k0 reads
    variants = {}
    xa = x.copy()
    xa[far] = full_scale
    variants["a neighbour's sample at the far end of the reach"] = fm.fused_audio(xa, h, DA, k0, n, row0=row)
    variants["row phase wrong by 4"] = fm.fused_audio(x, h, DA, k0, n, row0=row + 4)
    xc = x.copy()
    assert xc[far + 1] != 0
    xc[far + 1] = 0
    variants["a zeroed history sample at the far end of the reach"] = fm.fused_audio(xc, h, DA, k0, n, row0=row)
    for name, v in variants.items():
        assert (bits(v) != bits(y)).any(), name + ": the same bits"
        assert rms(v, y) < 2e-6, (name, rms(v, y))
        assert np.abs(oracle.pcm16(v).astype(np.int32) - oracle.pcm16(y).astype(np.int32)).max() <= 1, name
    xd = x.copy()
    xd[DA * k0 - 1] = full_scale
    assert rms(fm.fused_audio(xd, h, DA, k0, n, row0=row), y) > 1e-3


def test_mixer_and_combine_helpers():
    sf = np.array([1.5, -3.0, 2.0 ** -140, 7.0], F32)
    pll = np.array([0.25, -1.0, 0.5, 0.1, 9.0], F32)
    np.testing.assert_array_equal(fm.mixer(sf, pll), np.array([0.75, 6.0, 2.0 ** -140, (F32(7.0) * F32(0.1)) * 2], F32))
    l, r = fm.combine(np.array([1.0, 2.0 ** -30], F32), np.array([1.0, 1.0], F32))
    assert l.tolist() == [2.0, 1.0] and r.tolist() == [0.0, 1.0]


def define_list(path, name):
    with open(path) as f:
        src = f.read()
    m = re.search(r"#define\s+" + name + r"\(X\)\s*((?:X\(\s*\d+\s*\)\s*)+)", src)
    assert m, f"{name} not found in {path}"
    return [int(a) for a in re.findall(r"X\(\s*(\d+)\s*\)", m.group(1))]


def stereo_out_shapes():
    with open(os.path.join(CSRC, "kernels_stereo.hip")) as f:
        src = f.read()
    body = src[src.index("int stereo_out_launch("):]
    m = re.search(r"#undef X", body)
    tail = body[:m.start()]
    line = re.findall(r"^\s*((?:X\(\s*\d+\s*,\s*\d+\s*\)\s*)+)$", tail, re.M)
    assert len(line) == 1, line
    return [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", line[0])]


def test_gpu_tests_cover_every_shape():
    """The GPU file's shape lists are the kernels' dispatch lists: a new shape cannot ship without its exact test."""
    import test_gpu_fir_exact as g
    ks, cs = os.path.join(CSRC, "kernels_stereo.hip"), os.path.join(CSRC, "kernels_bank.hip")
    assert sorted(define_list(ks, "FMRX_BPF_CASES")) == sorted(g.BPF_TAPS)
    assert sorted(parse_cases(os.path.join(CSRC, "kernels_audio.hip"), "FMRX_AUDIO_CASES")) == sorted(g.AUDIO_SHAPES)
    assert sorted(stereo_out_shapes()) == sorted(g.STEREO_OUT_SHAPES)
    assert sorted(define_list(cs, "CHS_BPF_CASES")) == sorted(g.CHS_BPF_TAPS)
    assert sorted(parse_cases(cs, "CHS_OUT_CASES")) == sorted(g.CHS_OUT_SHAPES)
    # and every listed shape is run
    assert {t[2] for _, t, _, _ in g.BANK_CONFIGS} == set(g.CHS_BPF_TAPS)
    assert {(t[1], {0: 5, 1: 6}[m]) for m, t, _, _ in g.BANK_CONFIGS} == set(g.CHS_OUT_SHAPES)
    assert {s for _, a, s in g.STEREO_CASES} == set(g.BPF_TAPS)
    assert {(a, {0: 5, 1: 6}[m]) for m, a, _ in g.STEREO_CASES if m in (0, 1)} == set(g.STEREO_OUT_SHAPES)


def test_mono_bank_tests_cover_every_shape_and_state_the_launch_rule():
    """tests/test_gpu_mono_banks_exact.py runs every fused shape, the full list at 101/101 taps in both modes, and its
    groups_per_wave() is launch_resample's rule: the loop as kernels_bank.hip has it, and the thresholds it gives."""
    import test_gpu_mfma_exact as m
    import test_gpu_mono_banks_exact as g
    assert {c[:4] for c in g.FUSED_BANK_CASES} == set(m.FUSED_CASES)
    for shape in ((101, 10, 101, 5), (101, 5, 101, 6)):
        assert {c[4:] for c in g.FUSED_BANK_CASES if c[:4] == shape} == {(n, k) for n in (1, 7, 70) for k in g.BLOCK_KINDS}
    with open(os.path.join(CSRC, "kernels_bank.hip")) as f:
        src = f.read()
    assert "while (gpw > NW && cgs * periods * ((b.res_groups + gpw - 1) / gpw) * NW < 8192) gpw = (gpw + 1) / 2;" in src
    assert "gpw = (gpw + NW - 1) / NW * NW;" in src and "template <bool STEREO> constexpr int kRW = STEREO ? 3 : 7;" in src
    assert "test_gpu_mono_banks_exact.py" in src

    def first(U, stereo, groups):
        return next(X for X in range(1, 2000) if g.groups_per_wave(64 * X, 1, U, stereo)[1] >= groups)
    assert (first(441, False, 2), first(441, False, 3), first(147, False, 2), first(441, True, 2)) == (147, 293, 586, 171)
    assert g.groups_per_wave(65, 7, 441, False) == (14, 1) and g.groups_per_wave(40000, 7, 147, False)[1] > 1


def test_resample_chain_equals_sequential_exact_fma():
    """resample_chain (chs_resample_lanes_kernel of the fast bank) against a scalar loop of exact fmas in the reference's
    resampler order (src/filter.cpp:191-223: j ascending), then y + fl(y U)."""
    rng = np.random.default_rng(9)
    for T, U, D, delay in [(21, 3, 5, 2), (35, 7, 4, 0), (14, 7, 10, 3)]:
        x = rng.standard_normal(40).astype(F32)
        h = rng.standard_normal(T).astype(F32)
        y = fm.resample_chain(x, h, U, D, delay)
        want = []
        for k in range(len(x) * U // D):
            m = k * D
            ph = m % U
            n0 = (m - ph) // U
            acc = F32(0.0)
            for j, n in enumerate(range(ph, T, U)):
                i = n0 - j - delay
                acc = exact_fma(x[i] if i >= 0 else F32(0.0), h[n], acc)
            want.append(acc + acc * F32(U))
        np.testing.assert_array_equal(bits(y), bits(np.array(want, F32)), err_msg=f"T={T} U={U} D={D}")


def test_resample_chain_differs_from_reference_order(oracle):
    """On a mode-2 discriminator stream the fma resampler differs from the oracle's convolve_block_resample_fir somewhere
    and stays within 1e-5 of the peak of the result."""
    x, p = demod_stream(oracle, 2, nblk=2)
    h = oracle.impulse_response_lpf(float(p.if_Fs * p.audio_upsamp), 16e3, p.audio_taps)
    U, D = p.audio_upsamp, p.audio_decim
    y = fm.resample_chain(x, h, U, D)
    ref, _ = oracle.convolve_block_resample_fir(x, h, np.zeros(p.audio_taps - 1, F32), D, U)
    assert (bits(y) != bits(ref)).any()
    assert np.max(np.abs(y.astype(np.float64) - ref)) <= 1e-5 * np.max(np.abs(ref))
