"""A plain numpy model of the packed-FMA FIR kernels: one fused multiply-add per tap, the taps in a fixed order.

The kernels it models (the order of each read from its loop, checked on the GPU by tests/test_gpu_fir_exact.py):
  bpf_pair_kernel (kernels_stereo.hip)       both band-pass filters, D = 1, taps DESCENDING (oldest window sample first)
  stereo_out_kernel (kernels_stereo.hip)     both audio FIRs, taps ascending, the mono one `delay` samples back
  audio_fir_kernel (kernels_audio.hip)       polyphase: branch p = 0 .. D-1, inside it m = p, p + D, ...; tap n = T-1-m
  chs_bpf_kernel, chs_out_kernel (kernels_bank.hip, fast bank)      taps ascending (newest window sample first)
  chs_resample_lanes_kernel (fast bank, modes 2/3)   the reference's resampler order (j ascending), one fma per tap

Every model takes the STREAM the kernel read -- the concatenation of a tap over the calls, zeros before the stream's
start -- and computes output k as acc = +0.0f; acc = fmaf(x[D k - n - delay], h[n], acc) for n in the given order.
Products and sums are rounded once per step, as v_fma_f32 / v_pk_fma_f32 round them.  No GPU involved."""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def fmaf(a, b, c):
    """fmaf on float32 arrays, exactly rounded (round to nearest, ties to even).

    a*b is exact in float64 (48 bits); TwoSum gives s = RN64(a*b + c) and its exact error e.  RN32(s) is RN32(a*b + c)
    unless s lies exactly on a float32 midpoint with e != 0: then the exact value lies on e's side of it."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(F64) * b.astype(F64)
    return _round_sum(p, c.astype(F64))


def _round_sum(p, c):
    """RN32(p + c) for float64 p, c whose exact sum is what is wanted (p exact product, c a float32).

    s = RN64(p + c) rounds to the right float32 unless s sits exactly on a float32 midpoint (its 29 low mantissa bits
    10...0) or in the float32 subnormal range: only those few go through _fix_midpoints."""
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    r = s.astype(F32)
    low = s.view(np.uint64) & np.uint64(0x1FFFFFFF)
    cand = (low == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -125)
    if cand.any():
        i = np.flatnonzero(cand)
        r.flat[i] = _fix_midpoints(np.ravel(p)[i] if np.ndim(p) else np.full(len(i), p),
                                   np.ravel(c)[i] if np.ndim(c) else np.full(len(i), c))
    return r


def _fix_midpoints(p, c):
    """RN32(p + c) for 1-d float64 arrays: TwoSum gives s = RN64(p + c) and its exact error e; RN32(s) is the answer
    unless s lies exactly on a float32 midpoint with e != 0: then the exact value lies on e's side of it."""
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    d = s - r.astype(F64)
    # a midpoint sits half a float32 spacing from r (a quarter when r is a power of two and s lies below it in magnitude)
    sp = np.spacing(np.abs(r)).astype(F64)
    ad = np.abs(d)
    cand = (e != 0) & (d != 0) & ((ad == 0.5 * sp) | (ad == 0.25 * sp))
    if cand.any():
        i = np.flatnonzero(cand)
        ri, si, di, ei = r[i], s[i], d[i], e[i]
        nb = np.nextafter(ri, np.where(di > 0, F32(np.inf), F32(-np.inf)))
        mid = (ri.astype(F64) + nb.astype(F64)) * 0.5 == si
        take = mid & ((ei > 0) == (di > 0))
        r[i[take]] = nb[take]
    return r


def fmaf_via_f64(a, b, c):
    """The plain route float32(float64(a*b) + c): rounded twice, wrong where the float64 sum lands on a float32 midpoint."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


# ---- tap orders ---------------------------------------------------------------------------------------------------
def ascending(T):
    return list(range(T))


def descending(T):
    return list(range(T - 1, -1, -1))


def polyphase(T, D):
    """audio_fir_kernel's order (au_step): branch p = 0 .. D-1, inside it table entries m = p, p + D, ... (m < T), each
    holding h[T-1-m]."""
    return [T - 1 - m for p in range(D) for m in range(p, T, D)]


ORDERS = {"bpf_pair_kernel": lambda T, D: descending(T),
          "stereo_out_kernel": lambda T, D: ascending(T),
          "audio_fir_kernel": polyphase,
          "chs_bpf_kernel": lambda T, D: ascending(T),
          "chs_out_kernel": lambda T, D: ascending(T)}


# ---- the chain ----------------------------------------------------------------------------------------------------
def _columns(x, T, D, delay, k0, n_out):
    """xp (float64, zeros in front) and base such that xp[base + D k - n] = x[D (k0 + k) - n - delay]."""
    x = np.asarray(x, F32)
    front = T - 1 + delay
    xp = np.concatenate([np.zeros(front, F64), x.astype(F64)])
    base = front + D * k0 - delay
    assert base - (T - 1) >= 0 and base + D * (n_out - 1) < len(xp), "outputs outside the stream"
    return xp, base


def fma_chain(x, h, order, decim=1, delay=0, k0=0, n_out=None):
    """y[k] = the fmaf chain over taps `order` of output k0 + k: acc = fmaf(x[D k - n - delay], h[n], acc), acc = +0.
    x: the whole stream from its start (samples before it are 0)."""
    h = np.asarray(h, F32)
    T, D = len(h), int(decim)
    if n_out is None:
        n_out = len(x) // D - k0
    xp, base = _columns(x, T, D, delay, k0, n_out)
    acc = np.zeros(n_out, F64)
    stop = base + D * (n_out - 1) + 1
    for n in order:
        acc = _round_sum(xp[base - n:stop - n:D] * F64(h[n]), acc).astype(F64)
    return acc.astype(F32)


def ref_chain(x, h, decim=1, delay=0, k0=0, n_out=None):
    """The reference's order (src/filter.cpp: convolveBlockFIR / convolveBlockFastFIR): acc = fl(acc + fl(h[n] x)), n
    ascending -- numpy's float32 operations are correctly rounded, so this IS that order."""
    h = np.asarray(h, F32)
    T, D = len(h), int(decim)
    if n_out is None:
        n_out = len(x) // D - k0
    xp, base = _columns(x, T, D, delay, k0, n_out)
    xp = xp.astype(F32)
    acc = np.zeros(n_out, F32)
    stop = base + D * (n_out - 1) + 1
    for n in range(T):
        acc = acc + xp[base - n:stop - n:D] * h[n]
    return acc


def fir64(x, h, decim=1, delay=0, k0=0, n_out=None):
    """-> (the float64 FIR, sum_n |h[n] x[D k - n - delay]|) of the same outputs."""
    h = np.asarray(h, F32).astype(F64)
    T, D = len(h), int(decim)
    if n_out is None:
        n_out = len(x) // D - k0
    xp, base = _columns(x, T, D, delay, k0, n_out)
    y, a = np.zeros(n_out, F64), np.zeros(n_out, F64)
    stop = base + D * (n_out - 1) + 1
    for n in range(T):
        t = xp[base - n:stop - n:D] * h[n]
        y += t
        a += np.abs(t)
    return y, a


def gamma(T):
    """gamma_T = T u / (1 - T u), u = 2^-24: |chain - exact FIR| <= gamma_T sum |h x| for any order of T fmas."""
    return T * U / (1 - T * U)


# ---- the kernels ---------------------------------------------------------------------------------------------------
def bpf_pair(demod, h_st, h_car, k0=0, n_out=None):
    """bpf_pair_kernel: (stereo_filt, carrier_filt) of the stream's samples k0 .. k0 + n_out - 1, taps descending."""
    T = len(h_st)
    return (fma_chain(demod, h_st, descending(T), 1, 0, k0, n_out),
            fma_chain(demod, h_car, descending(T), 1, 0, k0, n_out))


def mixer(stereo_filt, pll):
    """(stereo_filt[g] * PLL[g]) * 2 in float32 (src/project.cpp:246-248); pll: PLL[0] (the state's lastOut) first."""
    sf = np.asarray(stereo_filt, F32)
    return (sf * np.asarray(pll, F32)[:len(sf)]) * F32(2.0)


def combine(st, mono):
    """left = st + mono, right = mono - st (src/project.cpp:278-279)."""
    st, mono = np.asarray(st, F32), np.asarray(mono, F32)
    return st + mono, mono - st


def resample_chain(x, h, upsamp, decim, delay=0, n_out=None):
    """chs_resample_lanes_kernel of the FAST bank (modes 2/3): the reference's resampler (src/filter.cpp:191-223) with
    one fmaf per tap in its order.  Output k: m = k D, ph = m mod U, n0 = (m - ph) / U;
    acc = fmaf(x[n0 - j - delay], h[ph + j U], acc) for j = 0, 1, ... while ph + j U < T; then y = acc + fl(acc U)."""
    x = np.asarray(x, F32)
    h = np.asarray(h, F32).astype(F64)
    T, Uu, D = len(h), int(upsamp), int(decim)
    if n_out is None:
        n_out = len(x) * Uu // D
    m = np.arange(n_out, dtype=np.int64) * D
    ph = m % Uu
    n0 = (m - ph) // Uu
    front = (T + Uu - 1) // Uu + delay
    xp = np.concatenate([np.zeros(front, F64), x.astype(F64)])
    acc = np.zeros(n_out, F64)
    for j in range((T + Uu - 1) // Uu):
        n = ph + j * Uu
        ok = n < T
        i = front + n0 - j - delay
        acc = np.where(ok, _round_sum(xp[i] * h[np.minimum(n, T - 1)], acc), acc)
    a = acc.astype(F32)
    return a + a * F32(Uu)


def audio_pair(demod, mix, h, decim, delay, order, k0=0, n_out=None):
    """The two audio FIRs of stereo_out_kernel / chs_out_kernel: (mono on demod `delay` back, stereo on the mixer)."""
    return (fma_chain(demod, h, order, decim, delay, k0, n_out), fma_chain(mix, h, order, decim, 0, k0, n_out))


# ---- the f32 matrix-core FIRs (v_mfma_f32_16x16x4_f32) ------------------------------------------------------------
# One v_mfma_f32_16x16x4_f32 adds, to every C element, the 4 products of its row of A and column of B as a chain of
# fmaf in K order: D = fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))), each rounded once, C/D never flushed.
# MFMA_K_ORDER is that order of the K index inside one instruction; the models take it as a parameter so that another
# order can be tried against the hardware without touching them.
MFMA_K_ORDER = (0, 1, 2, 3)


def _padded(x, front, back):
    return np.concatenate([np.zeros(front, F64), np.asarray(x, F32).astype(F64), np.zeros(back, F64)])


def audio_mfma_ksteps(taps, decim):
    """AK of FuCfg / audio_mfma_ksteps (fe_mfma_host.hpp): K-steps covering the TA-1+15 DA+1 samples of a column, in
    whole groups of 4."""
    return ((taps - 1) + 15 * decim + 1 + 15) // 16 * 4


def audio_mfma_table(h, decim):
    """audio_mfma_build_table: [AK][64], lane (row i = lane & 15, kq = lane >> 4) of K-step j holds the tap that row i
    applies to window sample w = 16 (j/4) + 4 kq + j%4, h[DA i + TA-1 - w], 0 outside the filter."""
    h = np.asarray(h, F32)
    TA, DA = len(h), int(decim)
    AK = audio_mfma_ksteps(TA, DA)
    tab = np.zeros((AK, 64), F32)
    for j in range(AK):
        for lane in range(64):
            w = 16 * (j // 4) + 4 * (lane >> 4) + j % 4
            k = DA * (lane & 15) + TA - 1 - w
            if 0 <= k < TA:
                tab[j, lane] = h[k]
    return tab


def fused_audio(x, h, decim, k0=0, n_out=None, kq_order=MFMA_K_ORDER, row0=0):
    """The audio FIR inside mono_fused_kernel (kernels_fe_mfma.hip): outputs k0 .. k0 + n_out - 1 of ONE block whose
    first output is k0 (row i of an output = its index in the block mod 16).  Output o, row i: window sample w carries
    tap DA i + TA-1 - w and meets x[DA o - (DA i + TA-1 - w)].  K-step j feeds y0 (j even) or y1 (j odd), each an fmaf
    chain from +0 over j ascending, kq in `kq_order` inside each MFMA, padding K-steps included; y = y0 + y1 (one f32
    add).  x: the discriminator stream from its start (samples before it are 0).

    row0: the row of output k0 where the block does not start a launch -- the fused mono bank (bank.hip) runs all
    slots as one launch, so channel c's first kept output sits at row (c * slot_audio + junk_audio) mod 16.  The row
    decides which K-steps carry an output's taps, hence which products land in the even and which in the odd chain.  It
    is the block that starts row0 outputs earlier, those outputs dropped (16 DA zeros in front keep them in the
    stream: in front of the filter's reach only zero taps meet them)."""
    TA, DA = len(h), int(decim)
    if n_out is None:
        n_out = len(x) // DA - k0
    row0 = int(row0)
    assert 0 <= row0 < 16
    if row0:
        xz = np.concatenate([np.zeros(16 * DA, F32), np.asarray(x, F32)])
        return fused_audio(xz, h, DA, k0 + 16 - row0, n_out + row0, kq_order)[row0:]
    tab = audio_mfma_table(h, decim)
    assert n_out == 0 or DA * (k0 + n_out - 1) < len(x), "outputs outside the stream"
    AK = tab.shape[0]
    n16 = -(-n_out // 16)
    # the 16 outputs 16 t + i of a column share its window: x[DA (k0 + 16 t) - (TA-1) + w] for every row i
    front = TA
    xp = _padded(x, front, 16 * DA + 4 * AK)
    base = front + DA * k0 - (TA - 1)
    step = 16 * DA
    y = [np.zeros((n16, 16), F64), np.zeros((n16, 16), F64)]
    for j in range(AK):
        for kq in kq_order:
            w = 16 * (j // 4) + 4 * kq + j % 4
            xv = xp[base + w:base + w + step * (n16 - 1) + 1:step]
            y[j & 1] = _round_sum(xv[:, None] * tab[j, 16 * kq:16 * kq + 16].astype(F64), y[j & 1]).astype(F64)
    return (y[0].astype(F32) + y[1].astype(F32)).ravel()[:n_out]


def row_phase_changes_bits(decim, row0):
    """Whether fused_audio(row0=r) can differ in bits from row0 = 0.  Row i applies tap k to window sample
    w = DA i + TA-1 - k; K-step j = 4 (w / 16) + w % 4 and kq = (w / 4) % 4 place it.  Moving an output by r rows moves
    every w by DA r: a multiple of 16 moves every tap by whole groups of four K-steps -- the same chain (j keeps its
    parity), the same order inside it, only zero products in front -- so the bits stay.  At DA = 6 that is r = 8 (and
    r = 12 equals r = 4); at DA = 5 no phase but 0."""
    return (int(decim) * int(row0)) % 16 != 0


def resample_mfma_plan(taps, upsamp, decim):
    """The host-side geometry of resample_mfma_kernel (resample_mfma_host.hpp), or None where the kernel does not apply:
    per 16-row output tile m its top input offset, the K-steps in sixteens (KS4), the tile groups (m0, m1, lo, pieces)
    and the staging loads per thread (NL) of both instances."""
    U, D = int(upsamp), int(decim)
    J = (taps + U - 1) // U
    if D % 4 or U < 16:
        return None
    ntiles = (U + 15) // 16
    top, K = [], 0
    for m in range(ntiles):
        r_last = min(16 * m + 15, U - 1)
        bmax = r_last * D // U
        b0 = 16 * m * D // U
        top.append((bmax + 1 + 3) // 4 * 4 - 1)
        K = max(K, top[m] - b0 + J)
    KS4 = max(8, (K + 31) // 32 * 2)
    if KS4 > 16:
        return None
    groups = []
    for m in range(0, ntiles, 4):
        m1 = min(m + 4, ntiles)
        lo = top[m] - 16 * KS4 + 1
        pieces = (top[m1 - 1] - lo + 1) // 4
        if pieces > 160:
            return None
        groups.append((m, m1, lo, pieces))
    max_pieces = max(g[3] for g in groups)
    nl = max(4, (max_pieces + 15) // 16)
    return dict(J=J, K=K, KS4=KS4, top=top, groups=groups, max_pieces=max_pieces, nl16=nl, nl_elem=(nl + 1) // 2 * 2)


def resample_mfma_image(h, upsamp, decim, plan=None):
    """The tap image [tile][lane][K-step]: lane (row i = lane & 15, kq = lane >> 4) of tile m, K-step ks <-> K index
    w = 16 (ks/4) + 4 kq + ks%4 = input top[m] - w of the period; output r = 16 m + i (< U) takes h[ph + j U] there,
    ph = r D mod U, j = floor(r D / U) - (top - w), 0 outside the filter."""
    h = np.asarray(h, F32)
    U, D, T = int(upsamp), int(decim), len(h)
    plan = plan or resample_mfma_plan(T, U, D)
    KS4, J, top = plan["KS4"], plan["J"], plan["top"]
    img = np.zeros((len(top), 64, 4 * KS4), F32)
    for m in range(len(top)):
        for lane in range(64):
            i, kq = lane & 15, lane >> 4
            r = 16 * m + i
            if r >= U:
                continue
            ph, bi = r * D % U, r * D // U
            for ks in range(4 * KS4):
                w = 16 * (ks // 4) + 4 * kq + ks % 4
                j = bi - (top[m] - w)
                if 0 <= j < J and ph + j * U < T:
                    img[m, lane, ks] = h[ph + j * U]
    return img


def resample_mfma(x, h, upsamp, decim, delay=0, k0=0, n_out=None, kq_order=MFMA_K_ORDER, image=None):
    """resample_mfma_kernel (kernels_resample.hip): output k = q U + r (period q, r = 16 m + i) is ONE fmaf chain from +0
    over K-steps ks = 4 jj + e (jj ascending, then e), kq in `kq_order` inside each MFMA, of image[m][i + 16 kq][ks]
    times the input x[q D + top[m] - w - delay]; then out = acc + fl(acc U).  x: the stream from its start (0 before
    it); k0 and n_out whole periods (blocks are)."""
    h = np.asarray(h, F32)
    U, D, T = int(upsamp), int(decim), len(h)
    plan = resample_mfma_plan(T, U, D)
    img = resample_mfma_image(h, U, D, plan) if image is None else image
    KS4, top = plan["KS4"], plan["top"]
    if n_out is None:
        n_out = len(x) // D * U - k0
    assert k0 % U == 0 and n_out % U == 0, "whole periods"
    q0, nq = k0 // U, n_out // U
    front = 16 * KS4 + delay
    xp = _padded(x, front, D + 16 * KS4 + max(top) + 4)
    out = np.zeros((nq, len(top) * 16), F32)
    for m in range(len(top)):
        # the 16 rows of tile m in period q read the same inputs x[q D + top[m] - w]
        base = front + q0 * D + top[m] - delay
        acc = np.zeros((nq, 16), F64)
        for jj in range(KS4):
            for e in range(4):
                for kq in kq_order:
                    w = 16 * jj + 4 * kq + e
                    xv = xp[base - w:base - w + D * (nq - 1) + 1:D]
                    acc = _round_sum(xv[:, None] * img[m, 16 * kq:16 * kq + 16, 4 * jj + e].astype(F64), acc).astype(F64)
        out[:, 16 * m:16 * m + 16] = acc.astype(F32)
    a = out[:, :U].ravel()
    return a + a * F32(U)


def resample64(x, h, upsamp, decim, delay=0):
    """-> (the float64 resampler (1 + U) sum_j h[ph + j U] x[n0 - j - delay], (1 + U) sum_j |h x|) of every output."""
    x = np.asarray(x, F32)
    h = np.asarray(h, F32).astype(F64)
    T, U, D = len(h), int(upsamp), int(decim)
    n_out = len(x) * U // D
    m = np.arange(n_out, dtype=np.int64) * D
    ph, n0 = m % U, m // U
    J = (T + U - 1) // U
    xp = _padded(x, J + delay, 0)
    y, s = np.zeros(n_out, F64), np.zeros(n_out, F64)
    for j in range(J):
        n = ph + j * U
        t = np.where(n < T, xp[J + delay + n0 - j - delay] * h[np.minimum(n, T - 1)], 0.0)
        y += t
        s += np.abs(t)
    return y * (1 + U), s * (1 + U)


def resample_mfma_reach_ok(plan, decim, front, back):
    """resample_mfma_reach_ok: 16-byte piece staging stays within `front` samples in front of the block, `back` behind."""
    lo = [g[2] for g in plan["groups"]]
    return -min(0, *lo) <= front and max(0, *lo) + 64 * plan["nl16"] - int(decim) <= back
