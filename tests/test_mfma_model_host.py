"""The fma-chain models of the f32 matrix-core FIRs (tests/_fir_model.py: fused_audio, resample_mfma) against plain
sequential loops of exact fmas, the float64 FIR and the other paths' orders; their tap images against the library's
host code (dumped by tests/cpp/mfma_tables_dump.cpp); and the coverage of tests/test_gpu_mfma_exact.py.  No GPU
involved."""
import os
import re
import subprocess

import numpy as np
import pytest

import _fir_model as fm
from test_fir_model_host import bits, demod_stream, exact_fma

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "software-defined-radio_amd", "csrc")
F32 = np.float32
AUDIO_SHAPES = [(101, 5), (101, 6), (13, 5), (13, 6)]


# ---- the models against sequential exact fmas ------------------------------------------------------------------------
def stream_with_edges(rng, n, scale=1.0):
    """Random samples with signed zeros, subnormals and tiny values mixed in."""
    x = (rng.standard_normal(n) * scale).astype(F32)
    k = rng.integers(0, 6, n)
    x[k == 0] = F32(0.0)
    x[k == 1] = F32(-0.0)
    tiny = rng.integers(-5000, 5000, n) * np.ldexp(1.0, -149)
    x[k == 2] = tiny[k == 2].astype(F32)                     # subnormal
    return x


def fused_sequential(x, h, DA, k0, n_out, kq_order=fm.MFMA_K_ORDER, row0=0):
    """mono_fused_kernel's audio FIR read straight off its description, one exact fma at a time: output o (row
    i = (o - k0 + row0) mod 16), K-step j, K index kq: window sample w = 16 (j/4) + 4 kq + j%4, tap k = DA i + TA-1 - w (0 outside
    the filter) times x[DA o - k] (0 outside the stream); y0 takes even j, y1 odd j; y = y0 + y1."""
    TA = len(h)
    AK = fm.audio_mfma_ksteps(TA, DA)
    out = []
    for o in range(k0, k0 + n_out):
        i = (o - k0 + row0) % 16
        y = [F32(0.0), F32(0.0)]
        for j in range(AK):
            for kq in kq_order:
                w = 16 * (j // 4) + 4 * kq + j % 4
                k = DA * i + TA - 1 - w
                n = DA * o - k
                xv = x[n] if 0 <= n < len(x) else F32(0.0)
                y[j & 1] = exact_fma(xv, h[k] if 0 <= k < TA else F32(0.0), y[j & 1])
        out.append(F32(y[0] + y[1]))
    return np.array(out, F32)


def resample_sequential(x, h, U, D, delay, periods):
    """resample_mfma_kernel read off its description: output q U + r, tile m = r / 16, ph = r D mod U, bi = floor(r D / U);
    K-step ks = 4 jj + e, kq: w = 16 jj + 4 kq + e, j = bi - (top[m] - w), tap h[ph + j U] where 0 <= j < J and
    ph + j U < T (else 0) times x[q D + top[m] - w - delay] (0 outside the stream); out = acc + fl(acc U)."""
    T = len(h)
    plan = fm.resample_mfma_plan(T, U, D)
    J, KS4, top = plan["J"], plan["KS4"], plan["top"]
    out = []
    for q in periods:
        for r in range(U):
            m, ph, bi = r // 16, r * D % U, r * D // U
            acc = F32(0.0)
            for jj in range(KS4):
                for e in range(4):
                    for kq in range(4):
                        w = 16 * jj + 4 * kq + e
                        j = bi - (top[m] - w)
                        tap = h[ph + j * U] if 0 <= j < J and ph + j * U < T else F32(0.0)
                        n = q * D + top[m] - w - delay
                        acc = exact_fma(x[n] if 0 <= n < len(x) else F32(0.0), tap, acc)
            out.append(acc + acc * F32(U))
    return np.array(out, F32)


@pytest.mark.parametrize("TA,DA", AUDIO_SHAPES)
def test_fused_audio_equals_sequential_exact_fma(TA, DA):
    rng = np.random.default_rng(TA * 10 + DA)
    x = stream_with_edges(rng, DA * 60 + 7)
    h = rng.standard_normal(TA).astype(F32)
    h[0] = F32(0.0)                                          # as the Hann-windowed taps
    h[1] = F32(np.ldexp(1.0, -140))
    for k0, n_out in ((0, 19), (13, 37 if TA == 13 else 21)):
        got = fm.fused_audio(x, h, DA, k0, n_out)
        want = fused_sequential(x, h, DA, k0, n_out)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"TA {TA} DA {DA} k0 {k0}")
        # the fused bank's row phases: the first output of the block sits at row 4, 8 or 12 of its launch
        for row0 in (4, 8, 12):
            got = fm.fused_audio(x, h, DA, k0, n_out, row0=row0)
            want = fused_sequential(x, h, DA, k0, n_out, row0=row0)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"TA {TA} DA {DA} k0 {k0} row0 {row0}")
    # a stream of tiny values: products and sums underflow to signed zeros and subnormals
    xs = (stream_with_edges(rng, DA * 40) * F32(2.0 ** -100)).astype(F32)
    hs = (rng.standard_normal(TA) * 2.0 ** -40).astype(F32)
    got = fm.fused_audio(xs, hs, DA, 3, 20)
    want = fused_sequential(xs, hs, DA, 3, 20)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert (np.abs(want) < np.finfo(F32).tiny).any()


def test_fused_audio_kq_order_parameter():
    """Another order inside the MFMA is another model: the parameter reaches the chain."""
    rng = np.random.default_rng(3)
    x, h = rng.standard_normal(600).astype(F32), rng.standard_normal(13).astype(F32)
    rev = (3, 2, 1, 0)
    np.testing.assert_array_equal(bits(fm.fused_audio(x, h, 5, 0, 40, rev)), bits(fused_sequential(x, h, 5, 0, 40, rev)))
    assert (bits(fm.fused_audio(x, h, 5, 0, 100, rev)) != bits(fm.fused_audio(x, h, 5, 0, 100))).any()


@pytest.mark.parametrize("T,U,D,delay", [(5 * 19, 19, 40, 0), (7 * 19, 19, 40, 3), (3 * 33, 33, 20, 6), (13 * 147, 147, 800, 50)])
def test_resample_mfma_equals_sequential_exact_fma(T, U, D, delay):
    rng = np.random.default_rng(T + U + D)
    periods = 4 if U < 100 else 2
    x = stream_with_edges(rng, D * periods + 5)
    h = rng.standard_normal(T).astype(F32)
    h[0] = F32(0.0)
    got = fm.resample_mfma(x, h, U, D, delay, U, (periods - 1) * U)
    want = resample_sequential(x, h, U, D, delay, range(1, periods))
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"T {T} U {U} D {D}")
    if U < 100:
        got = fm.resample_mfma(x, h, U, D, delay, 0, periods * U)
        np.testing.assert_array_equal(bits(got), bits(resample_sequential(x, h, U, D, delay, range(periods))))


# ---- against float64 and the other paths' orders -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_fused_audio_within_gamma_and_differs_from_other_orders(oracle, mode):
    """Within gamma(4 AK + 1) sum|h x| of the float64 FIR on the production taps; on the discriminator stream different
    from the two-kernel path's polyphase chain, the ascending chain and the reference's order."""
    x, p = demod_stream(oracle, mode)
    DA = p.audio_decim
    for TA in (101, 13):
        h = oracle.impulse_response_lpf(float(p.if_Fs), 16e3, TA)
        y = fm.fused_audio(x, h, DA)
        y64, a = fm.fir64(x, h, DA)
        assert (np.abs(y.astype(np.float64) - y64) <= fm.gamma(4 * fm.audio_mfma_ksteps(TA, DA) + 1) * a).all()
        for other in (fm.fma_chain(x, h, fm.polyphase(TA, DA), DA), fm.fma_chain(x, h, fm.ascending(TA), DA),
                      fm.ref_chain(x, h, DA)):
            assert (bits(y) != bits(other)).any()


@pytest.mark.parametrize("mode", [2, 3])
def test_resample_mfma_within_gamma_and_differs_from_other_orders(oracle, mode):
    """Within gamma(16 KS4 + 2) sum|h x| (1 + U) of the float64 resampler; different from the fast bank's order
    (resample_chain) and from the reference's separately rounded one (what resample_exact runs)."""
    x, p = demod_stream(oracle, mode, nblk=2)
    U, D = p.audio_upsamp, p.audio_decim
    x = x[:len(x) // D * D]
    for base in (101, 13):
        h = oracle.impulse_response_lpf(float(p.if_Fs * U), 16e3, base * U)
        y = fm.resample_mfma(x, h, U, D)
        y64, a = fm.resample64(x, h, U, D)
        assert (np.abs(y.astype(np.float64) - y64) <= fm.gamma(16 * fm.resample_mfma_plan(len(h), U, D)["KS4"] + 2) * a).all()
        ref, _ = oracle.convolve_block_resample_fir(x, h, np.zeros(len(h) - 1, F32), D, U)
        assert (bits(y) != bits(fm.resample_chain(x, h, U, D))).any() and (bits(y) != bits(ref[:len(y)])).any()


# ---- the tap images against the library's host code ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mfma") / "mfma_tables_dump"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "cpp", "mfma_tables_dump.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def resample_margins():
    with open(os.path.join(CSRC, "fmrx_internal.hpp")) as f:
        m = re.search(r"constexpr int kResampleFront = (\d+), kResampleBack = (\d+);", f.read())
    assert m
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("TA,DA", AUDIO_SHAPES)
def test_audio_table_equals_library(oracle, dump_exe, tmp_path, TA, DA):
    """fused_audio's tap image is audio_mfma_build_table's (fe_mfma_host.hpp), on the production taps."""
    h = oracle.impulse_response_lpf({5: 240e3, 6: 288e3}[DA], 16e3, TA)
    h.tofile(tmp_path / "h.f32")
    r = subprocess.run([str(dump_exe), "audio", str(tmp_path / "h.f32"), str(TA), str(DA), str(tmp_path / "t.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = np.fromfile(tmp_path / "t.f32", F32)
    model = fm.audio_mfma_table(h, DA)
    assert model.shape[0] == {(101, 5): 44, (101, 6): 48, (13, 5): 24, (13, 6): 28}[(TA, DA)]
    np.testing.assert_array_equal(bits(lib), bits(model.ravel()))


def fused_cases():
    with open(os.path.join(CSRC, "kernels_fe_mfma.hip")) as f:
        src = f.read()
    m = re.search(r"#define\s+FMRX_FUSED_CASES\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m
    return [tuple(int(v) for v in t) for t in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]


def resample_configs():
    """(mode, base taps, U, D) of every matrix-core resampler the pipeline runs: modes 2/3 x the audio tap counts of the
    fused shapes (FMRX_FUSED_CASES)."""
    taps = sorted({ta for _, _, ta, _ in fused_cases()}, reverse=True)
    return [(m, t, u, d) for m, (u, d) in ((2, (147, 800)), (3, (441, 3200))) for t in taps]


@pytest.mark.parametrize("mode,base,U,D", resample_configs())
def test_resample_image_equals_library(oracle, dump_exe, tmp_path, mode, base, U, D):
    """resample_mfma's geometry and tap image are resample_mfma_geometry's (resample_mfma_host.hpp, what
    resample_mfma_plan uploads), on the production taps; and so are KS4, the staging loads and the reach."""
    T = base * U
    h = oracle.impulse_response_lpf({2: 240e3, 3: 320e3}[mode] * U, 16e3, T)
    h.tofile(tmp_path / "h.f32")
    front, back = resample_margins()
    r = subprocess.run([str(dump_exe), "resample", str(tmp_path / "h.f32"), str(T), str(U), str(D), str(front), str(back),
                        str(tmp_path / "img.f32"), str(tmp_path / "geo.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(tmp_path / "geo.txt") as f:
        head, tops, groups = [[int(v) for v in line.split()] for line in f.read().splitlines()]
    plan = fm.resample_mfma_plan(T, U, D)
    assert head == [plan["KS4"], plan["K"], plan["max_pieces"], plan["nl16"], plan["nl_elem"],
                    int(fm.resample_mfma_reach_ok(plan, D, front, back))]
    assert tops == plan["top"] and groups == [v for g in plan["groups"] for v in g]
    assert head[5] == 1                                      # the pipeline's mono calls stage 16-byte pieces
    np.testing.assert_array_equal(bits(np.fromfile(tmp_path / "img.f32", F32)), bits(fm.resample_mfma_image(h, U, D, plan).ravel()))


# ---- coverage of the GPU file ---------------------------------------------------------------------------------------------
def switch_instances(fn):
    """The X(...) instance lists of the switches in kernels_resample.hip's function `fn`, in order."""
    with open(os.path.join(CSRC, "kernels_resample.hip")) as f:
        src = f.read()
    body = src[src.index("static int " + fn + "("):]
    body = body[:body.index("\n}\n")]
    return [[int(v) for v in re.findall(r"X\((\d+)\)", line)] for line in re.findall(r"^\s*((?:X\(\d+\)\s*)+)$", body, re.M)]


def test_gpu_mfma_tests_cover_every_instance():
    """tests/test_gpu_mfma_exact.py runs every fused shape, and its resampler calls reach every (KS4, NL, staging)
    instance the pipeline uses; those instances exist in the dispatch lists."""
    import test_gpu_mfma_exact as g
    fc = fused_cases()
    assert len(fc) == 12 and sorted(fc) == sorted(g.FUSED_CASES)
    assert {(d, da) for _, d, _, da in fc} == {(10, 5), (5, 6)}
    ks4_list, = switch_instances("resample_mfma_launch")
    nl_elem_list, nl16_list = switch_instances("resample_mfma_launch_nl")
    used = {}
    for mode, base, U, D in resample_configs():
        plan = fm.resample_mfma_plan(base * U, U, D)
        used[(mode, base)] = (plan["KS4"], plan["nl16"], plan["nl_elem"])
        assert plan["KS4"] in ks4_list and plan["nl16"] in nl16_list and plan["nl_elem"] in nl_elem_list
    # the instances of the issue's table, derived above from the plan's formulas
    assert used == {(2, 101): (12, 8, 8), (2, 13): (8, 7, 8), (3, 101): (14, 9, 10), (3, 13): (8, 8, 8)}
    # 16-byte staging: the mono calls; element staging: the stereo calls (all-pass delay not a multiple of 4, the mixer)
    assert {(m, t) for m, t, _, _ in g.RESAMPLE_CASES} == set(used)
    assert {(m, t) for m, t, _ in g.STEREO_RS_CASES} == set(used)
    assert all(((s - 1) // 2) % 4 for _, _, s in g.STEREO_RS_CASES)
    # period counts: the minimum, not whole blocks of 16, several blocks per workgroup (resample_chains 1 and 2)
    per = {(m, t): {(n, c) for mm, tt, n, c in g.RESAMPLE_CASES if (mm, tt) == (m, t)} for m, t in used}
    for s in per.values():
        assert {(64, 0), (77, 0), (171, 0), (400, 0), (1007, 1), (1007, 2)} <= s
