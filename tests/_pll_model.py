"""A plain numpy model of the stereo PLL's FAST recurrence, written from the arithmetic the kernels document
(csrc/kernels_pll.hip: pll_step_clean, pll_step<kFast>, nco_out<kFast>; the file is built under fp contract(off)).

For an ordinary input sample (1e-20 < |v| < 1e20: pll_ordinary) one step is plain IEEE arithmetic:

    half = fr >= 0 ? 0.5f : -0.5f;  turn = v > 0 ? 0 : half;  eD = (turn - fr) * 6.2831853f          (f32, two roundings)
    integ = integ + Ki*eD;  phase = (phase + Kp*eD) + integ;  off += 1                                (f32, every op rounded)
    trigArg = (float)(w*(double)off + (double)phase)                                                  (f64 mul, f64 add, one f32 rounding)
    rev = (double)trigArg * 0.15915494309189533577;  fr = (float)(rev - rint(rev))

Any other sample takes the library path: eI = v*cos, eQ = v*(-1*sin) with the HARDWARE sine / cosine of fr, then glibc's
atan2f.  The model covers v = +-0 and +-inf there, where only the signs of cos(2 pi fr) and sin(2 pi fr) matter: eD is
glibc's atan2f (through ctypes on this host's libm) of the signed zeros / infinities.  A step is UNDETERMINED -- the
model cannot know what the device computes -- where those signs are in doubt (fr within 2^-20 of +-0.25 or +-0.5; of 0
too for an infinite v), and for any other non-ordinary v (NaN, denormal-small, huge): there the hardware functions'
magnitudes enter.  Near fr = 0 a zero v is determined: cos > 0, and the two candidates +0 / -0 for eD only set the sign
of a zero added to the integrator, which starts at +0 and so stays +0 or moves the same way either way.

Loop constants as the reference's fmPLL derives them (and make_coef in kernels_pll.hip): Kp = normBandwidth * 2.666f,
Ki = (normBandwidth * normBandwidth) * 3.555f in float; w = 2 pi * (double)(freq / Fs), freq / Fs a float division.

The NCO (nco_out<kFast>, chs_nco_kernel<false>, chs_out_kernel of the fast bank) is cos(2 pi r) with
r = (float)(rev - rint(rev)), rev = (double)(trigArg * ncoScale + phaseAdjust) / 2 pi: the model returns r, the device's
v_cos_f32(r) is compared with float64 cos(2 pi r) to within NCO_EPS."""
from __future__ import annotations

import ctypes
import ctypes.util
import math
from dataclasses import dataclass

import numpy as np

F32, F64 = np.float32, np.float64
TWO_PI_F = F32(6.28318530717958647692)       # the float literal the kernels multiply by
INV_2PI = 0.15915494309189533577             # a double
EDGE = 2.0 ** -20                            # |fr - edge| below this: the hardware sign of cos / sin is not known

# |v_cos_f32(r) - cos(2 pi r)| over r in [-0.5, 0.5] revolutions: 1.25e-7 measured on an MI355X over 1.7e7 NCO samples
# (tests/test_gpu_pll_exact.py prints it); the bound is 4 x that
NCO_EPS = 5.0e-7


@dataclass
class Coef:
    Kp: np.float32
    Ki: np.float32
    w: float
    nco_scale: np.float32
    phase_adjust: np.float32


def coef(freq=19e3, Fs=240e3, nco_scale=2.0, phase_adjust=0.0, norm_bandwidth=0.01) -> Coef:
    """fmPLL's constants (src/project.cpp:237 passes 19e3, if_Fs, 2, 0, 0.01)."""
    nb = F32(norm_bandwidth)
    Kp = F32(nb * F32(2.666))
    Ki = F32(F32(nb * nb) * F32(3.555))
    w = 2 * math.pi * float(F32(F32(freq) / F32(Fs)))
    return Coef(Kp, Ki, w, F32(nco_scale), F32(phase_adjust))


@dataclass
class State:
    """Per lane: integrator, phase estimate, trigOffset (float32, as the reference carries them) and fr, the reduced angle
    of the last trigArg in revolutions (what the fast bank carries in state slot 6)."""
    integ: np.ndarray
    phase: np.ndarray
    off: np.ndarray
    fr: np.ndarray

    def copy(self) -> "State":
        return State(self.integ.copy(), self.phase.copy(), self.off.copy(), self.fr.copy())



def reset(lanes=1) -> State:
    """The start-of-stream state {0, 0, 1, 0, 1, 0}: fr = 0 is the angle of (fbI, fbQ) = (1, 0)."""
    z = np.zeros(lanes, F32)
    return State(z.copy(), z.copy(), z.copy(), z.copy())


_atan2f = None
_atan2f_cache: dict = {}


def libm_atan2f(y, x) -> np.float32:
    """atan2f of this host's C library (glibc 2.35 here, pinned by tests/test_libm_exact.py), one pair."""
    global _atan2f
    if _atan2f is None:
        f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").atan2f
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        _atan2f = f
    y, x = F32(y), F32(x)
    key = (int(np.array(y).view(np.uint32)), int(np.array(x).view(np.uint32)))
    r = _atan2f_cache.get(key)
    if r is None:
        r = _atan2f_cache[key] = F32(_atan2f(y, x))
    return r


def ordinary(v) -> np.ndarray:
    a = np.abs(np.asarray(v, F32))
    return (a > F32(1e-20)) & (a < F32(1e20))


def closed_form_detector(v, fr) -> np.ndarray:
    """eD of an ordinary sample: -t (v > 0) or -t turned by pi (v < 0), t = 2 pi fr; float32, as pll_step_clean."""
    v, fr = np.asarray(v, F32), np.asarray(fr, F32)
    half = np.where(fr >= 0, F32(0.5), F32(-0.5)).astype(F32)
    turn = np.where(v > 0, F32(0.0), half).astype(F32)
    return ((turn - fr) * TWO_PI_F).astype(F32)


def library_detector(v, fr):
    """eD of a non-ordinary sample and whether it is undetermined (see the module docstring), lane by lane."""
    v, fr = np.atleast_1d(np.asarray(v, F32)), np.atleast_1d(np.asarray(fr, F32))
    t = 2 * math.pi * fr.astype(F64)
    fbI, fbQ = np.cos(t).astype(F32), np.sin(t).astype(F32)
    with np.errstate(invalid="ignore"):
        eI = (v * fbI).astype(F32)
        eQ = (v * (F32(-1) * fbQ)).astype(F32)
    f = np.abs(fr.astype(F64))
    near_sign_edge = (np.abs(f - 0.25) < EDGE) | (0.5 - f < EDGE)
    zero, inf = v == 0, np.isinf(v)
    und = ~(zero | inf) | near_sign_edge | (inf & (f < EDGE))
    eD = np.zeros(len(v), F32)
    for i in np.flatnonzero(~und):
        eD[i] = libm_atan2f(eQ[i], eI[i])
    return eD, und


def run(v, c: Coef, st: State | None = None):
    """Walk the recurrence over v [lanes, n] (or [n]) from state st (default: reset).

    Returns (trig [lanes, n] float32 -- the raw trigArg of every step --, the final State, und [lanes] -- the first
    undetermined step of each lane, -1 if none; a lane's outputs from that step on are not the model's to state)."""
    v = np.asarray(v, F32)
    one = v.ndim == 1
    v = np.atleast_2d(v)
    L, n = v.shape
    st = reset(L) if st is None else st.copy()
    integ, phase, off, fr = st.integ, st.phase, st.off, st.fr
    off64 = off.astype(F64)
    trig = np.empty((L, n), F32)
    und = np.full(L, -1, np.int64)
    ordv = ordinary(v)
    plain = ordv.all(axis=0)
    pos = v > 0
    Ki, Kp, w = c.Ki, c.Kp, c.w
    h_pos, h_neg, zero = F32(0.5), F32(-0.5), F32(0.0)
    for k in range(n):
        turn = np.where(pos[:, k], zero, np.where(fr >= zero, h_pos, h_neg))
        eD = (turn - fr) * TWO_PI_F
        if not plain[k]:
            odd = np.flatnonzero(~ordv[:, k])
            e_lib, u = library_detector(v[odd, k], fr[odd])
            eD[odd] = e_lib
            for i in odd[u]:
                if und[i] < 0:
                    und[i] = k
        integ = integ + Ki * eD
        phase = (phase + Kp * eD) + integ
        t = (w * (off64 + (k + 1)) + phase.astype(F64)).astype(F32)
        rev = t.astype(F64) * INV_2PI
        fr = (rev - np.rint(rev)).astype(F32)
        trig[:, k] = t
    off = (off64 + n).astype(F32)
    out = State(integ.astype(F32), phase.astype(F32), off, fr)
    return (trig[0] if one else trig), out, (und[0] if one else und)


def nco_arg(trig, c: Coef) -> np.ndarray:
    """r of the NCO: a = trigArg * ncoScale + phaseAdjust (float32), r = (float)(rev - rint(rev)), rev = (double)a / 2 pi."""
    a = (np.asarray(trig, F32) * c.nco_scale + c.phase_adjust).astype(F32)
    rev = a.astype(F64) * INV_2PI
    return (rev - np.rint(rev)).astype(F32)


def nco(trig, c: Coef) -> np.ndarray:
    """cos(2 pi r) in float64: what v_cos_f32(r) approximates to within NCO_EPS."""
    return np.cos(2 * math.pi * nco_arg(trig, c).astype(F64))


def carrier_sign(y) -> np.ndarray:
    """The byte the fast bank's band-pass kernel stores for the PLL (chs_bpf_kernel): +1 / -1 for an ordinary sample, else 0."""
    y = np.asarray(y, F32)
    return np.where(ordinary(y), np.where(y > 0, 1, -1), 0).astype(F32)
