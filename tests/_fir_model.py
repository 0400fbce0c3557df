"""A plain numpy model of the packed-FMA FIR kernels: one fused multiply-add per tap, the taps in a fixed order.

The kernels it models (the order of each read from its loop, checked on the GPU by tests/test_gpu_fir_exact.py):
  bpf_pair_kernel (kernels_stereo.hip)       both band-pass filters, D = 1, taps DESCENDING (oldest window sample first)
  stereo_out_kernel (kernels_stereo.hip)     both audio FIRs, taps ascending, the mono one `delay` samples back
  audio_fir_kernel (kernels_audio.hip)       polyphase: branch p = 0 .. D-1, inside it m = p, p + D, ...; tap n = T-1-m
  chs_bpf_kernel, chs_out_kernel (channels_stereo.hip, fast bank)   taps ascending (newest window sample first)
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
    """RN32(p + c) for float64 p, c whose exact sum is what is wanted (p exact product, c a float32)."""
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
        ri, si, di, ei = r.flat[i], s.flat[i], d.flat[i], e.flat[i]
        nb = np.nextafter(ri, np.where(di > 0, F32(np.inf), F32(-np.inf)))
        mid = (ri.astype(F64) + nb.astype(F64)) * 0.5 == si
        take = mid & ((ei > 0) == (di > 0))
        r.flat[i[take]] = nb[take]
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
