"""software-defined-radio_amd -- MI355X-native FM receiver DSP hot path.

Python host mirror of the reference's operator interface for this path: the
free functions of ``include/filter.h:18-43`` and ``include/iofunc.h:36`` of
mnigm2001/Software-Defined-Radio (same names, argument order and meaning; numpy
arrays in place of ``std::vector<float>&``, outputs returned instead of passed
by reference), plus the pipeline handle that replaces ``src/project.cpp``'s
thread bodies.  Everything here is a thin ctypes binding over the C ABI of
``lib/libfmrx.so`` (``include/fmrx.h``); all compute runs in HIP kernels on the
GPU.  There is no CPU fallback: without the built library this module raises on
import, and without a GPU every compute call raises ``FmrxError`` (ENODEV).

The directory name contains '-', so import it with::

    import importlib; fmrx = importlib.import_module("software-defined-radio_amd")
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMRX_LIB") or os.path.join(_HERE, "lib", "libfmrx.so")   # FMRX_LIB: A/B a development build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fmrx.h")

OK, EINVAL, ENODEV, EHIP, ENOMEM = 0, 1, 2, 3, 4
PCM_WRAP, PCM_SATURATE = 1, 0
TAPS = {"if_i": 0, "if_q": 1, "demod": 2, "mono_filt": 3, "carrier_filt": 4, "stereo_filt": 5, "pll": 6, "mixer": 7,
        "stereo_final": 8, "trig_arg": 9}


class FmrxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fmrx error {code}: {msg}")
        self.code = code


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C software-defined-radio_amd/csrc`). There is no Python/CPU fallback.")



# libfmrx.so and PyTorch can be loaded in either order: the library records its HIP / HSA runtime dependencies
# by the unversioned names torch's own libraries use, so ld.so maps ONE runtime whichever comes first
# (csrc/Makefile; tests/test_load_order.py runs both orders on the GPU).
lib = C.CDLL(LIB_PATH)

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
_i16p = np.ctypeslib.ndpointer(dtype=np.int16, flags="C_CONTIGUOUS")
_vp, _sz, _int, _uint, _flt = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_float


class Params(C.Structure):
    """struct fmrx_params == the reference's PARAMS + mode table (src/project.cpp:17-27, 424-427)."""
    _fields_ = [("mode", _int), ("rf_Fs", _int), ("if_Fs", _int), ("audio_Fs", _flt), ("rf_decim", _int),
                ("audio_decim", _int), ("audio_upsamp", _int), ("rf_taps", _int), ("audio_taps", _int),
                ("stereo_taps", _int), ("block_bytes", _int)]


def _sig(name, args, res=_int):
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = args, res
    return fn


_sig("fmrx_version", [], C.c_char_p)
_sig("fmrx_last_error", [], C.c_char_p)
_sig("fmrx_device_count", [])
_sig("fmrx_set_device", [_int])
_sig("fmrx_set_option", [C.c_char_p, C.c_long])
_sig("fmrx_get_option", [C.c_char_p, C.POINTER(C.c_long)])
_sig("fmrx_host_alloc", [C.POINTER(_vp), _sz])
_sig("fmrx_host_free", [_vp])
_sig("fmrx_impulse_response_lpf", [_flt, _flt, C.c_ushort, _f32p])
_sig("fmrx_band_pass", [_flt, _flt, _flt, C.c_ushort, _f32p])
_sig("fmrx_u8_to_f32", [_u8p, _sz, _f32p])
_sig("fmrx_deinterleave", [_f32p, _sz, _f32p, _f32p])
_sig("fmrx_convolve_fir", [_f32p, _f32p, _sz, _f32p, _sz])
_sig("fmrx_convolve_block_fir", [_f32p, _f32p, _sz, _f32p, _sz, _f32p])
_sig("fmrx_convolve_block_fast_fir", [_f32p, _f32p, _sz, _f32p, _sz, _f32p, _uint])
_sig("fmrx_convolve_block_resample_fir", [_f32p, _f32p, _sz, _f32p, _sz, _f32p, _uint, _uint])
_sig("fmrx_upsample", [_f32p, _sz, _f32p, _int])
_sig("fmrx_downsample", [_f32p, C.POINTER(_sz), _f32p, _sz, C.c_ushort])
_sig("fmrx_fm_demod", [_f32p, _f32p, _f32p, _sz, C.POINTER(_flt), C.POINTER(_flt)])
_sig("fmrx_all_pass", [_f32p, _sz, _f32p, _sz, _f32p])
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_sig("fmrx_fm_demod_arctan", [_f64p, _f64p, _f64p, _sz, C.POINTER(C.c_double)])
_sig("fmrx_fm_pll", [_f32p, _sz, _f32p, _f32p, _flt, _flt, _flt, _flt, _flt])


class PllParallelInfo(C.Structure):
    """struct fmrx_pll_parallel_info (include/fmrx.h)."""
    _fields_ = [("L", _int), ("W", _int), ("lti", _int), ("nseg", _sz), ("repaired", _uint), ("max_dphase", _flt),
                ("max_dinteg", _flt), ("tol_phase", _flt), ("tol_integ", _flt)]


PLL_RECORD_FLOATS = 9
_u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
_sig("fmrx_fm_pll_parallel", [_f32p, _sz, _f32p, _f32p, _flt, _flt, _flt, _flt, _flt, C.c_double, C.POINTER(PllParallelInfo),
                              _f32p, _u64p])
_sig("fmrx_stereo_mix", [_f32p, _f32p, _sz, _f32p])
_sig("fmrx_stereo_combine", [_f32p, _f32p, _sz, _f32p, _f32p])
_sig("fmrx_pcm16", [_f32p, _sz, _i16p, _int])
_sig("fmrx_deemph_design", [C.c_double, C.c_double, C.POINTER(_flt), C.POINTER(_flt)])
_sig("fmrx_deemph", [_f32p, _f32p, _sz, _sz, _sz, _flt, _flt, _f32p, C.POINTER(_uint)])
_sig("fmrx_deemph_dev", [_vp, _vp, _sz, _sz, _sz, _flt, _flt, _vp, _vp, _vp])
_ull = C.c_ulonglong
_sig("fmrx_pipeline_set_deemphasis", [_vp, C.c_double])
_sig("fmrx_pipeline_deemph_diagnostics", [_vp, C.POINTER(_ull), C.POINTER(_ull)])
_sig("fmrx_channels_set_deemphasis", [_vp, C.c_double])
_sig("fmrx_channels_deemph_diagnostics", [_vp, C.POINTER(_ull), C.POINTER(_ull)])
_sig("fmrx_estimate_psd", [_f32p, _f32p, _f32p, _sz, _flt, _int])
_sig("fmrx_diag_libm", [_int, _f32p, _vp, _sz, _f32p])
_sig("fmrx_diag_demod_fast", [_f32p, _f32p, _sz, _flt, _flt, _int])
_sig("fmrx_diag_stream_read_dev", [_vp, _sz, _int, _vp])
_sig("fmrx_mode_params", [_int, _int, _int, _int, C.POINTER(Params)])
_sig("fmrx_pipeline_create", [C.POINTER(_vp), C.POINTER(Params), _int, _sz, _int])
_sig("fmrx_pipeline_destroy", [_vp])
_sig("fmrx_pipeline_reset", [_vp])
_sig("fmrx_pipeline_n_if", [_vp, _sz], _sz)
_sig("fmrx_pipeline_n_audio", [_vp, _sz], _sz)
_sig("fmrx_pipeline_process", [_vp, _u8p, _sz, _vp, _vp, _int])
_sig("fmrx_pipeline_process_dev", [_vp, _vp, _sz, _vp, _vp, _int, _vp])
_sig("fmrx_pipeline_submit", [_vp, _vp, _sz, _vp, _vp, _int])
_sig("fmrx_pipeline_wait", [_vp])
_sig("fmrx_pipeline_read_tap", [_vp, _int, _vp, C.POINTER(_sz)])
_sig("fmrx_pipeline_state_size", [_vp], _sz)
_sig("fmrx_pipeline_get_state", [_vp, _f32p, _sz])
_sig("fmrx_pipeline_set_state", [_vp, _f32p, _sz])
_sig("fmrx_pipeline_last_timing", [_vp, _f32p])
_sig("fmrx_pipeline_timing_sum", [_vp, _f32p, C.POINTER(_int), _int])
_sig("fmrx_pipeline_set_profiling", [_vp, _int])
_sig("fmrx_pipeline_set_force_generic", [_vp, _int])
_sig("fmrx_pipeline_set_keep_intermediates", [_vp, _int])
_sig("fmrx_pipeline_set_option", [_vp, C.c_char_p, C.c_long])
_sig("fmrx_pipeline_pll_diagnostics", [_vp, C.POINTER(_uint), C.POINTER(_flt), C.POINTER(_flt)])
_sig("fmrx_channels_create", [C.POINTER(_vp), C.POINTER(Params), _int, _sz, _int])
_sig("fmrx_channels_create_ex", [C.POINTER(_vp), C.POINTER(Params), _int, _int, _int, _sz, _int])
_sig("fmrx_channels_read_tap", [_vp, _int, _int, _vp, C.POINTER(_sz)])
_sig("fmrx_channels_destroy", [_vp])
_sig("fmrx_channels_n_audio", [_vp], _sz)
_sig("fmrx_channels_input_layout", [_vp, C.POINTER(_vp), C.POINTER(_sz)])
_sig("fmrx_channels_reset", [_vp, _int])
_sig("fmrx_channels_load_dev", [_vp, _vp, _vp])
_sig("fmrx_channels_process", [_vp, _u8p, _vp, _vp, _int])
_sig("fmrx_channels_process_dev", [_vp, _vp, _vp, _int, _vp])
class RdsParams(C.Structure):
    _fields_ = [("if_Fs", _int), ("taps", _int), ("upsamp", _int), ("decim", _int), ("sps", _int), ("rrc_taps", _int)]


_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_sig("fmrx_rds_mode_params", [_int, C.POINTER(RdsParams)])
_sig("fmrx_rds_create", [C.POINTER(_vp), C.POINTER(RdsParams), _sz, _int])
_sig("fmrx_rds_destroy", [_vp])
_sig("fmrx_rds_reset", [_vp])
_sig("fmrx_rds_n_out", [_vp, _sz], _sz)
_sig("fmrx_rds_process", [_vp, _f32p, _sz, _vp, _vp, _vp, C.POINTER(_sz), C.c_char_p])
_sig("fmrx_rds_process_dev", [_vp, _vp, _sz, _vp])
_sig("fmrx_rds_read_tap", [_vp, _int, _vp, C.POINTER(_sz)])
_sig("fmrx_rds_band_pass", [_int, C.c_double, C.c_double, C.c_double, _f64p])
_sig("fmrx_rds_imp_response", [_int, C.c_double, C.c_double, _f64p])
_sig("fmrx_rds_rrc", [C.c_double, _int, _f64p])
_sig("fmrx_rds_cdr", [_f64p, _sz, _int, _int, _f64p, _u8p, C.POINTER(_sz)])
_sig("fmrx_rds_diff_decode", [_u8p, _sz, _u8p])
_sig("fmrx_rds_frame_sync", [_u8p, _sz, C.c_char_p, C.POINTER(_sz)])
_sig("fmrx_rds_bank_create", [C.POINTER(_vp), C.POINTER(RdsParams), _int, _sz, _int])
_sig("fmrx_rds_bank_destroy", [_vp])
_sig("fmrx_rds_bank_reset", [_vp, _int])
_sig("fmrx_rds_bank_n_out", [_vp], _sz)
_sig("fmrx_rds_bank_max_bits", [_vp], _sz)
_sig("fmrx_rds_bank_process_dev", [_vp, _vp, _sz, _vp])
_sig("fmrx_rds_bank_collect", [_vp, _vp, _vp, _vp, _vp, _vp])
_sig("fmrx_rds_bank_process", [_vp, _f32p, _vp, _vp, _vp, _vp, _vp])
_sig("fmrx_rds_bank_read_tap", [_vp, _int, _int, _vp, C.POINTER(_sz)])
_sig("fmrx_rds_bank_set_stations", [_vp, _int])
_sig("fmrx_rds_bank_max_groups", [_vp], _sz)
_sig("fmrx_rds_bank_stations", [_vp, _vp, _vp, _vp])
_sig("fmrx_rds_station_create", [C.POINTER(_vp), _int])
_sig("fmrx_rds_station_destroy", [_vp])
_sig("fmrx_rds_station_reset", [_vp])
_sig("fmrx_rds_station_max_groups", [_vp, _sz], _sz)
_sig("fmrx_rds_station_feed_rrc", [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp])
_sig("fmrx_rds_station_feed_bits", [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), _vp])
_sig("fmrx_rds_station_set_correction", [_vp, _int])
_sig("fmrx_rds_station_ext_get", [_vp, _vp])
_sig("fmrx_rds_block_correct", [C.c_uint32, _int, _int, C.POINTER(C.c_uint16), C.POINTER(_int)])
_sig("fmrx_rds_bank_set_station_options", [_vp, _int, _int])
_sig("fmrx_rds_bank_stations_ext", [_vp, _vp])
_sig("fmrx_channels_demod_layout", [_vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_sz)])
_sig("fmrx_fe_fir_decim_u8", [_u8p, _sz, _f32p, _sz, _uint, _vp, _vp, _vp, _int])
_sig("fmrx_fe_plan_create", [C.POINTER(_vp), _f32p, _sz, _uint])
_sig("fmrx_fe_plan_destroy", [_vp])
_sig("fmrx_fe_plan_is_specialised", [_vp])
_sig("fmrx_fe_plan_history_bytes", [_vp], _sz)
_sig("fmrx_fe_run_dev", [_vp, _vp, _sz, _vp, _vp, _int, _vp])
_dbl = C.c_double
_sig("fmrx_tuner_design", [_f32p, _int, _dbl, _dbl, _dbl, C.POINTER(C.c_uint32), C.POINTER(_int), _i16p, _i16p])
_sig("fmrx_tuner_table", [_vp, _vp, C.POINTER(_sz)])
_sig("fmrx_tuner_create", [C.POINTER(_vp), _int, _f32p, _int, _int, _sz, _int])
_sig("fmrx_tuner_create_ex", [C.POINTER(_vp), _int, _f32p, _int, _int, _sz, _int, _int])
_sig("fmrx_tuner_design_rational", [_f32p, _int, _int, _dbl, _dbl, _dbl, C.POINTER(C.c_uint32), C.POINTER(_int), _i16p, _i16p])
_sig("fmrx_tuner_create_rational", [C.POINTER(_vp), _int, _int, _f32p, _int, _int, _sz, _int, _int])
_sig("fmrx_tuner_ratio", [_vp, C.POINTER(_int), C.POINTER(_int)])
_sig("fmrx_tuner_format", [_vp])
_sig("fmrx_tuner_sample_bytes", [_vp], _sz)


class TunerPlanInfo(C.Structure):
    """fmrx_tuner_plan_info: what one call of a Tuner launches (Tuner.plan)"""
    _fields_ = [("matrix", _int), ("tiles", _int), ("via_lds", _int), ("lds_bytes", _sz), ("n_steps", _int), ("steps_per_wg", _int),
                ("grid_x", _int), ("grid_y", _int)]


_sig("fmrx_tuner_plan", [_vp, _sz, C.POINTER(TunerPlanInfo)])
_sig("fmrx_tuner_destroy", [_vp])
_sig("fmrx_tuner_reset", [_vp])
_sig("fmrx_tuner_set_channel", [_vp, _int, _dbl, _dbl, _dbl])
_sig("fmrx_tuner_n_out_bytes", [_vp, _sz], _sz)
_sig("fmrx_tuner_process_dev", [_vp, _vp, _sz, _vp, _sz, _vp])
_sig("fmrx_tuner_process", [_vp, _vp, _sz, _u8p])
_sig("fmrx_tuner_levels", [_vp, _vp, _vp])
_sig("fmrx_meters_probes", [_f64p, C.POINTER(_int)])
_sig("fmrx_meters_table", [_dbl, _f64p, _f64p])
_sig("fmrx_meters_derive", [_dbl, _vp, _vp])
_sig("fmrx_meters_create", [C.POINTER(_vp), _dbl, _int, _int])
_sig("fmrx_meters_destroy", [_vp])
_sig("fmrx_meters_process_dev", [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp])
_sig("fmrx_meters_collect", [_vp, _vp])
_sig("fmrx_meters_process", [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp])


def _check(rc: int):
    if rc != OK:
        raise FmrxError(rc, lib.fmrx_last_error().decode(errors="replace"))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint8)


def version() -> str:
    return lib.fmrx_version().decode()


def device_count() -> int:
    return lib.fmrx_device_count()


def set_device(dev: int) -> None:
    _check(lib.fmrx_set_device(dev))


# option values that have names, per option (the same names as the table in csrc/options.cpp)
_OPTION_NAMES = {"fe_variant": {"mfma": 0, "valu": 1}, "tuner_variant": {"mfma": 0, "generic": 1},
                 "demod": {"discriminator": 0, "arctan": 1}}


def _option_value(name: str, value) -> int:
    names = _OPTION_NAMES.get(name, {})
    if isinstance(value, str) and value not in names:
        raise FmrxError(EINVAL, f"option {name}: '{value}' is not one of its named values {sorted(names)}")
    return names[value] if isinstance(value, str) else int(value)


def set_option(name: str, value) -> None:
    """Process-wide default of a run-time option (include/fmrx.h: fmrx_set_option); pipelines created
    afterwards start from it.  fe_variant also takes "mfma" / "valu", tuner_variant "mfma" / "generic",
    demod "discriminator" / "arctan"."""
    _check(lib.fmrx_set_option(name.encode(), _option_value(name, value)))


def get_option(name: str) -> int:
    v = C.c_long(0)
    _check(lib.fmrx_get_option(name.encode(), C.byref(v)))
    return v.value


def diagStreamRead(d_ptr, n_bytes, method=0, stream=None) -> None:
    """One pure streaming read of a device buffer (fmrx_diag_stream_read_dev), async on `stream`."""
    _check(lib.fmrx_diag_stream_read_dev(d_ptr, n_bytes, method, stream))


def hostAlloc(nbytes: int, dtype=np.uint8) -> np.ndarray:
    """A page-locked host buffer (fmrx_host_alloc) as a numpy array of `dtype`; free it with hostFree(arr)."""
    p = _vp()
    _check(lib.fmrx_host_alloc(C.byref(p), int(nbytes)))
    buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype)
    arr.flags.writeable = True
    _PINNED[arr.ctypes.data] = (p.value, buf)
    return arr


def hostFree(arr: np.ndarray) -> None:
    p, _ = _PINNED.pop(arr.ctypes.data)
    _check(lib.fmrx_host_free(p))


_PINNED: dict = {}


def deviceLibm(fn: str, a, b=None, flat=False) -> np.ndarray:
    """sinf / cosf / atan2f as the device evaluates csrc/glibc_libm.hpp (fmrx_diag_libm): test hook.
    flat: through the branch-free forms the receiver banks' PLL lanes run."""
    a = _f32(a)
    out = np.zeros(len(a), np.float32)
    bb = _f32(b) if b is not None else None
    _check(lib.fmrx_diag_libm({"sinf": 0, "cosf": 1, "atan2f": 2}[fn] + (3 if flat else 0), a,
                              bb.ctypes.data if bb is not None else None, len(a), out))
    return out


def deviceRcp(a) -> np.ndarray:
    """The hardware reciprocal (v_rcp_f32) of each element (fmrx_diag_libm, fn 6): test hook."""
    a = _f32(a)
    out = np.zeros(len(a), np.float32)
    _check(lib.fmrx_diag_libm(6, a, None, len(a), out))
    return out


def fmDemodFast(I, Q, prev_i=0.0, prev_q=0.0, bounded=False) -> np.ndarray:
    """The fast discriminator of the specialised paths (csrc/device_math.hpp: demod_fast; bounded: demod_fast_bounded)
    on the caller's IF (fmrx_diag_demod_fast): test hook."""
    I, Q = _f32(I), _f32(Q)
    iq = np.empty(2 * len(I), np.float32)
    iq[0::2], iq[1::2] = I, Q
    out = np.zeros(len(I), np.float32)
    _check(lib.fmrx_diag_demod_fast(out, iq, len(I), prev_i, prev_q, int(bool(bounded))))
    return out


# --------------------------------------------------------------------------
# filter.h mirror (reference names and argument order)
# --------------------------------------------------------------------------
def impulseResponseLPF(Fs, Fc, num_taps) -> np.ndarray:
    """filter.h:24 / filter.cpp:103-114 -> h[num_taps]."""
    h = np.zeros(num_taps, np.float32)
    _check(lib.fmrx_impulse_response_lpf(Fs, Fc, num_taps, h))
    return h


def bandPass(Fs, Fb, Fe, N_taps) -> np.ndarray:
    """filter.h:20 / filter.cpp:83-99 -> coeff[N_taps] (C++ argument order: Fs, Fb, Fe, taps)."""
    h = np.zeros(N_taps, np.float32)
    _check(lib.fmrx_band_pass(Fs, Fb, Fe, N_taps, h))
    return h


def convolveFIR(x, h) -> np.ndarray:
    """filter.h:26 / filter.cpp:118-130 -> y[len(x)+len(h)-1]."""
    x, h = _f32(x), _f32(h)
    y = np.zeros(len(x) + len(h) - 1, np.float32)
    _check(lib.fmrx_convolve_fir(y, x, len(x), h, len(h)))
    return y


def convolveBlockFIR(x, h, state):
    """filter.h:28 / filter.cpp:133-154 -> (y[len(x)], new_state)."""
    x, h, st = _f32(x), _f32(h), _f32(state).copy()
    if len(st) != len(h) - 1:
        raise FmrxError(EINVAL, "state must have len(h)-1 elements")
    y = np.zeros(len(x), np.float32)
    _check(lib.fmrx_convolve_block_fir(y, x, len(x), h, len(h), st))
    return y, st


def convolveBlockFastFIR(x, h, state, audio_decim):
    """filter.h:31 / filter.cpp:158-188 -> (y[len(x)//decim], new_state)."""
    x, h, st = _f32(x), _f32(h), _f32(state).copy()
    if len(st) != len(h) - 1:
        raise FmrxError(EINVAL, "state must have len(h)-1 elements")
    y = np.zeros(len(x) // max(int(audio_decim), 1), np.float32)
    _check(lib.fmrx_convolve_block_fast_fir(y, x, len(x), h, len(h), st, audio_decim))
    return y, st


def convolveBlockResampleFIR(x, h, state, audio_decim, audio_upsamp):
    """filter.h:34 / filter.cpp:191-223 -> (y[len(x)*U//D], new_state); state in the reference's layout."""
    x, h, st = _f32(x), _f32(h), _f32(state).copy()
    if len(st) != len(h) - 1:
        raise FmrxError(EINVAL, "state must have len(h)-1 elements")
    ny = (len(x) * int(audio_upsamp)) // max(int(audio_decim), 1)
    y = np.zeros(ny, np.float32)
    _check(lib.fmrx_convolve_block_resample_fir(y, x, len(x), h, len(h), st, audio_decim, audio_upsamp))
    return y, st


def upsample(x, up_rate) -> np.ndarray:
    x = _f32(x)
    xu = np.zeros(len(x) * up_rate, np.float32)
    _check(lib.fmrx_upsample(x, len(x), xu, up_rate))
    return xu


def downsample(x, ds_coeff) -> np.ndarray:
    x = _f32(x)
    out = np.zeros(len(x) + 1, np.float32)
    n = _sz(0)
    _check(lib.fmrx_downsample(out, C.byref(n), x, len(x), ds_coeff))
    return out[: n.value].copy()


def fmDemod(I, Q, prev_i=0.0, prev_q=0.0):
    """filter.h:41 / filter.cpp:248-266 -> (fm_demod, prev_i, prev_q)."""
    I, Q = _f32(I), _f32(Q)
    out = np.zeros(len(I), np.float32)
    pi, pq = _flt(prev_i), _flt(prev_q)
    _check(lib.fmrx_fm_demod(out, I, Q, len(I), C.byref(pi), C.byref(pq)))
    return out, pi.value, pq.value


def fmDemodArctan(I, Q, prev_phase=0.0):
    """model/fmSupportLib.py:502-531 -> (fm_demod, prev_phase): the Python model's arctangent demodulator, float64."""
    I, Q = np.ascontiguousarray(I, np.float64), np.ascontiguousarray(Q, np.float64)
    out = np.zeros(len(I), np.float64)
    ph = C.c_double(prev_phase)
    _check(lib.fmrx_fm_demod_arctan(out, I, Q, len(I), C.byref(ph)))
    return out, ph.value


def allPass(input_block, state_block):
    """filter.h:18 / filter.cpp:14-29 -> (output_block, new_state)."""
    x, st = _f32(input_block), _f32(state_block).copy()
    out = np.zeros(len(x), np.float32)
    _check(lib.fmrx_all_pass(x, len(x), st, len(st), out))
    return out, st


def fmPLL(PLLIn, state, freq, Fs, ncoScale=2.0, phaseAdjust=0.0, normBandwidth=0.01):
    """filter.h:22 / filter.cpp:32-80 -> (ncoOut[len+1], new_state[6])."""
    x, st = _f32(PLLIn), _f32(state).copy()
    if len(st) != 6:
        raise FmrxError(EINVAL, "PLL state has 6 elements")
    out = np.zeros(len(x) + 1, np.float32)
    _check(lib.fmrx_fm_pll(x, len(x), out, st, freq, Fs, ncoScale, phaseAdjust, normBandwidth))
    return out, st


def fmPllParallel(PLLIn, state, freq, Fs, ncoScale=2.0, phaseAdjust=0.0, normBandwidth=0.01, off_hint=-1.0):
    """The parallel-in-time fast PLL of the specialised stereo pipeline as a stage (fmrx_fm_pll_parallel), under the
    process-wide options pll_start / pll_warmup / pll_segment -> (ncoOut[len+1], new_state[6], info, records).

    info: dict of L, W, lti, nseg, repaired, max_dphase, max_dinteg, tol_phase, tol_integ and "mask" (bool per segment: the
    final mismatch flags).  records: dict of float32 arrays per segment -- "end" [nseg, 6], "basis" [nseg, 2] (the integrator
    and phase the segment's outputs were computed from) -- and "walks" [nseg] (times the repair walked the segment).  A block
    shorter than 4 L runs the serial kernel: nseg = 0, empty records."""
    x, st = _f32(PLLIn), _f32(state).copy()
    if len(st) != 6:
        raise FmrxError(EINVAL, "PLL state has 6 elements")
    out = np.zeros(len(x) + 1, np.float32)
    cap = len(x) // 32 + 2
    rec = np.zeros((cap, PLL_RECORD_FLOATS), np.float32)
    words = np.zeros(cap // 64 + 1, np.uint64)
    inf = PllParallelInfo()
    _check(lib.fmrx_fm_pll_parallel(x, len(x), out, st, freq, Fs, ncoScale, phaseAdjust, normBandwidth, off_hint, C.byref(inf), rec,
                                    words))
    info = {f: getattr(inf, f) for f, _ in PllParallelInfo._fields_}
    nseg = info["nseg"]
    info["lti"] = bool(info["lti"])
    info["mask"] = np.unpackbits(words.view(np.uint8), bitorder="little")[:nseg].astype(bool)
    rec = rec[:nseg]
    records = {"end": rec[:, :6].copy(), "basis": rec[:, 6:8].copy(), "walks": rec[:, 8].astype(np.int64)}
    return out, st, info, records


def stereoMix(stereo_filt, pll) -> np.ndarray:
    a, b = _f32(stereo_filt), _f32(pll)
    out = np.zeros(len(a), np.float32)
    _check(lib.fmrx_stereo_mix(a, b, len(a), out))
    return out


def stereoCombine(stereo_final, mono):
    a, b = _f32(stereo_final), _f32(mono)
    l, r = np.zeros(len(a), np.float32), np.zeros(len(a), np.float32)
    _check(lib.fmrx_stereo_combine(a, b, len(a), l, r))
    return l, r


def estimatePSD(samples, Fs, nfft=512):
    """fourier.h / fourier.cpp:44-128 -> (freq[nfft/2], psd_est[nfft/2] in dB); NFFT = 512 in the reference."""
    x = _f32(samples)
    freq, psd = np.zeros(nfft // 2, np.float32), np.zeros(nfft // 2, np.float32)
    _check(lib.fmrx_estimate_psd(freq, psd, x, len(x), Fs, nfft))
    return freq, psd


def readBlockData(raw_u8) -> np.ndarray:
    """iofunc.h:36 / iofunc.cpp:128-135, the conversion part: (u8-128)/128."""
    raw = _u8(raw_u8)
    out = np.zeros(len(raw), np.float32)
    _check(lib.fmrx_u8_to_f32(raw, len(raw), out))
    return out


def deinterleave(iq):
    iq = _f32(iq)
    n = len(iq) // 2
    I, Q = np.zeros(n, np.float32), np.zeros(n, np.float32)
    _check(lib.fmrx_deinterleave(iq, n, I, Q))
    return I, Q


def pcm16(audio, wrap=True) -> np.ndarray:
    a = _f32(audio)
    out = np.zeros(len(a), np.int16)
    _check(lib.fmrx_pcm16(a, len(a), out, PCM_WRAP if wrap else PCM_SATURATE))
    return out


def deemphasisCoeffs(Fs, tau_us):
    """(p, b0) of the de-emphasis filter as float32 (fmrx_deemph_design; host only, works without a GPU)."""
    p, b0 = _flt(0), _flt(0)
    _check(lib.fmrx_deemph_design(float(Fs), float(tau_us), C.byref(p), C.byref(b0)))
    return np.float32(p.value), np.float32(b0.value)


def deemphasis(x, p, b0, state=None, pitch=None):
    """The de-emphasis filter on rows x [rows, n] (or one row [n]) -> (y, state [rows, 2], missed segments).  pitch: floats
    between the rows on the device (default n)."""
    x = _f32(x)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    rows, n = x2.shape
    pitch = int(pitch or n)
    xs, ys = np.zeros((rows, pitch), np.float32), np.zeros((rows, pitch), np.float32)
    xs[:, :n] = x2
    st = np.zeros((rows, 2), np.float32) if state is None else _f32(state).reshape(rows, 2).copy()
    missed = _uint(0)
    _check(lib.fmrx_deemph(ys.reshape(-1), xs.reshape(-1), rows, n, pitch, float(p), float(b0), st.reshape(-1), C.byref(missed)))
    y = np.ascontiguousarray(ys[:, :n])
    return (y[0] if one else y), st, missed.value


def deemphasis_dev(d_y_ptr, d_x_ptr, rows, n, pitch, p, b0, d_state_ptr, d_missed_ptr, stream=None):
    """fmrx_deemph_dev on raw device addresses (state [rows, 2] float32, missed one uint64 the caller zeroes); async on `stream`."""
    _check(lib.fmrx_deemph_dev(d_y_ptr, d_x_ptr, rows, n, pitch, float(p), float(b0), d_state_ptr, d_missed_ptr, stream))


def frontEndFIR(iq_u8, h, decim, hist=None, force_generic=False):
    """Fused front end on host buffers -> (if_i, if_q, new_hist).  hist: u8[2*(taps-1)] or None."""
    iq, h = _u8(iq_u8), _f32(h)
    n = len(iq) // 2
    fi, fq = np.zeros(n // decim, np.float32), np.zeros(n // decim, np.float32)
    hb = None
    if hist is not None:
        hb = _u8(hist).copy()
        if len(hb) != 2 * (len(h) - 1):
            raise FmrxError(EINVAL, "hist must have 2*(taps-1) bytes")
    _check(lib.fmrx_fe_fir_decim_u8(iq, n, h, len(h), decim, hb.ctypes.data if hb is not None else None,
                                    fi.ctypes.data, fq.ctypes.data, 1 if force_generic else 0))
    return fi, fq, hb


def modeParams(mode, rf_taps=101, base_audio_taps=101, stereo_taps=101) -> Params:
    p = Params()
    _check(lib.fmrx_mode_params(mode, rf_taps, base_audio_taps, stereo_taps, C.byref(p)))
    return p


# --------------------------------------------------------------------------
# what every class that owns a library handle derives from
# --------------------------------------------------------------------------
class _Handle:
    """Owns self._h, a handle the library made; a subclass names the function that destroys it, or the _prefix of its
    fmrx_<_prefix>_* functions, which _call then finds by name."""
    _prefix = None
    _destroy = property(lambda self: f"fmrx_{self._prefix}_destroy")

    def _call(self, name, *args):
        _check(getattr(lib, f"fmrx_{self._prefix}_{name}")(self._h, *args))

    def close(self):
        if getattr(self, "_h", None) and lib is not None:  # lib is None during interpreter shutdown
            getattr(lib, self._destroy)(self._h)
            self._h = None

    __del__ = close


# --------------------------------------------------------------------------
# pipeline handle
# --------------------------------------------------------------------------
class Pipeline(_Handle):
    """RF_FrontEnd + RF_MONO / RF_STEREO of src/project.cpp as one device-resident pipeline."""
    _destroy = "fmrx_pipeline_destroy"

    def __init__(self, mode=0, channels=1, rf_taps=101, base_audio_taps=101, stereo_taps=101, max_block_bytes=None,
                 device=0, params: Params | None = None):
        self.params = params if params is not None else modeParams(mode, rf_taps, base_audio_taps, stereo_taps)
        self.channels = channels
        self.max_block_bytes = int(max_block_bytes or self.params.block_bytes)
        self._h = _vp()
        _check(lib.fmrx_pipeline_create(C.byref(self._h), C.byref(self.params), channels, self.max_block_bytes, device))

    def n_if(self, n_bytes):
        return lib.fmrx_pipeline_n_if(self._h, n_bytes)

    def n_audio(self, n_bytes):
        return lib.fmrx_pipeline_n_audio(self._h, n_bytes)

    def reset(self):
        _check(lib.fmrx_pipeline_reset(self._h))

    def set_profiling(self, on=True):
        _check(lib.fmrx_pipeline_set_profiling(self._h, int(on)))

    def set_keep_intermediates(self, on=True):
        """Also store the IF I/Q stream (read_tap('if_i'/'if_q')); the fused front end skips it by default."""
        _check(lib.fmrx_pipeline_set_keep_intermediates(self._h, int(on)))

    def pll_diagnostics(self):
        """(segments repaired serially, max accepted |dphase|, max accepted |dinteg|) of the parallel PLL."""
        r, dp, di = _uint(0), _flt(0), _flt(0)
        _check(lib.fmrx_pipeline_pll_diagnostics(self._h, C.byref(r), C.byref(dp), C.byref(di)))
        return r.value, dp.value, di.value

    def set_deemphasis(self, tau_us):
        """De-emphasis of the audio outputs with the time constant tau_us (50 or 75, any positive value); 0 = off (default)."""
        _check(lib.fmrx_pipeline_set_deemphasis(self._h, float(tau_us)))

    def deemph_diagnostics(self):
        """(segments checked, segments walked again) of the de-emphasis pass, cumulative since creation."""
        sg, ms = _ull(0), _ull(0)
        _check(lib.fmrx_pipeline_deemph_diagnostics(self._h, C.byref(sg), C.byref(ms)))
        return sg.value, ms.value

    def set_force_generic(self, on=True):
        """on: the bit-exact mode (reference evaluation order everywhere, serial PLL with glibc's functions)."""
        _check(lib.fmrx_pipeline_set_force_generic(self._h, int(on)))

    def set_option(self, name: str, value):
        """Per-handle run-time option (fmrx_pipeline_set_option); fe_variant also takes "mfma" / "valu"."""
        _check(lib.fmrx_pipeline_set_option(self._h, name.encode(), _option_value(name, value)))

    def process(self, iq_u8, want_pcm=True, wrap=True):
        """One block of interleaved u8 I/Q (host) -> dict(audio=..., [audio_l, audio_r], pcm16=...)."""
        iq = _u8(iq_u8)
        na = self.n_audio(len(iq))
        f = np.zeros(self.channels * na, np.float32)
        s = np.zeros(self.channels * na, np.int16) if want_pcm else None
        _check(lib.fmrx_pipeline_process(self._h, iq, len(iq), f.ctypes.data, s.ctypes.data if want_pcm else None,
                                         PCM_WRAP if wrap else PCM_SATURATE))
        out = {"pcm16": s}
        if self.channels == 1:
            out["audio"] = out["audio_l"] = f
        else:
            out["audio_l"], out["audio_r"] = f[:na], f[na:]
        return out

    def submit(self, iq_ptr, n_bytes, audio_ptr=None, pcm_ptr=None, wrap=True):
        """fmrx_pipeline_submit on raw HOST addresses (e.g. page-locked buffers from hostAlloc): enqueue and return."""
        _check(lib.fmrx_pipeline_submit(self._h, iq_ptr, n_bytes, audio_ptr, pcm_ptr, PCM_WRAP if wrap else PCM_SATURATE))

    def wait(self):
        """fmrx_pipeline_wait: the oldest submitted block's outputs are complete."""
        _check(lib.fmrx_pipeline_wait(self._h))

    def process_dev(self, d_iq_ptr, n_bytes, d_audio_ptr=None, d_pcm_ptr=None, wrap=True, stream=None):
        """Device-resident block: raw device addresses (e.g. torch.Tensor.data_ptr()); async on `stream`."""
        _check(lib.fmrx_pipeline_process_dev(self._h, d_iq_ptr, n_bytes, d_audio_ptr, d_pcm_ptr,
                                             PCM_WRAP if wrap else PCM_SATURATE, stream))

    def read_tap(self, name) -> np.ndarray:
        n = _sz(0)
        _check(lib.fmrx_pipeline_read_tap(self._h, TAPS[name], None, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(lib.fmrx_pipeline_read_tap(self._h, TAPS[name], out.ctypes.data, C.byref(n)))
        return out

    def get_state(self) -> np.ndarray:
        st = np.zeros(lib.fmrx_pipeline_state_size(self._h), np.float32)
        _check(lib.fmrx_pipeline_get_state(self._h, st, len(st)))
        return st

    def set_state(self, st):
        st = _f32(st)
        _check(lib.fmrx_pipeline_set_state(self._h, st, len(st)))

    def last_timing(self):
        t = np.zeros(4, np.float32)
        _check(lib.fmrx_pipeline_last_timing(self._h, t))
        return dict(front_end_ms=float(t[0]), audio_ms=float(t[1]), rest_ms=float(t[2]), total_ms=float(t[3]))

    def timing_sum(self, max_calls=0):
        """Sum of per-stage device times (ms) over the most recent profiled calls -> (dict, count)."""
        t, n = np.zeros(4, np.float32), _int(0)
        _check(lib.fmrx_pipeline_timing_sum(self._h, t, C.byref(n), max_calls))
        return dict(front_end_ms=float(t[0]), audio_ms=float(t[1]), rest_ms=float(t[2]), total_ms=float(t[3])), n.value


class Channels(_Handle):
    """N independent receivers (all four modes), the current block of all of them in one device call (fmrx_channels_*).

    audio_channels: 1 mono, 2 stereo (the reference's second command-line argument).  exact=True: every stage in the
    reference's float32 evaluation order, fmPLL as the serial recurrence with glibc's functions, one lane per channel --
    audio equals the compiled reference's bit for bit.  exact=False with audio_channels=2: the fast stereo bank (matrix-core
    front end, fma FIRs, the PLL's fast recurrence one lane per channel; the default stereo path's error envelope)."""
    _destroy = "fmrx_channels_destroy"

    def __init__(self, mode=0, n_channels=1, rf_taps=101, base_audio_taps=101, block_bytes=None, device=0, params: Params | None = None,
                 audio_channels=1, exact=False, stereo_taps=101):
        self.params = params if params is not None else modeParams(mode, rf_taps, base_audio_taps, stereo_taps)
        self.n_channels = int(n_channels)
        self.audio_channels = int(audio_channels)
        self.exact = bool(exact)
        self.block_bytes = int(block_bytes or self.params.block_bytes)
        self.device = int(device)
        self._h = _vp()
        _check(lib.fmrx_channels_create_ex(C.byref(self._h), C.byref(self.params), self.n_channels, self.audio_channels,
                                           int(self.exact), self.block_bytes, device))
        self.n_audio = lib.fmrx_channels_n_audio(self._h)

    def reset(self, channel=-1):
        _check(lib.fmrx_channels_reset(self._h, channel))

    def set_deemphasis(self, tau_us):
        """De-emphasis of every channel's audio with the time constant tau_us (50 or 75, any positive value); 0 = off (default)."""
        _check(lib.fmrx_channels_set_deemphasis(self._h, float(tau_us)))

    def deemph_diagnostics(self):
        """(segments checked, segments walked again) of the de-emphasis pass, cumulative since creation."""
        sg, ms = _ull(0), _ull(0)
        _check(lib.fmrx_channels_deemph_diagnostics(self._h, C.byref(sg), C.byref(ms)))
        return sg.value, ms.value

    def input_layout(self):
        """(device address of channel 0's block, pitch in bytes between channels)."""
        ptr, pitch = _vp(), _sz(0)
        _check(lib.fmrx_channels_input_layout(self._h, C.byref(ptr), C.byref(pitch)))
        return ptr.value, pitch.value

    def process(self, iq_u8, want_pcm=True, wrap=True):
        """iq_u8: [n_channels, block_bytes] uint8 (host) -> dict(audio=[n_channels, n_audio] f32, pcm16=... s16)."""
        iq = _u8(iq_u8).reshape(self.n_channels, self.block_bytes)
        st = self.audio_channels == 2
        f = np.zeros((self.n_channels, 2, self.n_audio) if st else (self.n_channels, self.n_audio), np.float32)
        s = None
        if want_pcm:
            s = np.zeros((self.n_channels, self.n_audio, 2) if st else (self.n_channels, self.n_audio), np.int16)
        _check(lib.fmrx_channels_process(self._h, iq.reshape(-1), f.ctypes.data, s.ctypes.data if want_pcm else None,
                                         PCM_WRAP if wrap else PCM_SATURATE))
        if st:   # stereo: audio [n_channels, 2, n_audio] (left, right), pcm16 [n_channels, n_audio, 2] interleaved L,R
            return {"audio": f, "audio_l": f[:, 0], "audio_r": f[:, 1], "pcm16": s}
        return {"audio": f, "pcm16": s}

    def read_tap(self, channel, name) -> np.ndarray:
        """One channel's intermediate of the last call ('demod'; stereo: 'carrier_filt' -- fast banks: its sign, -1 / 0 / +1 --,
        'stereo_filt', 'pll'; fast stereo banks of modes 0/1: 'trig_arg'); the fused mono bank of modes 0/1 keeps none."""
        n = _sz(0)
        _check(lib.fmrx_channels_read_tap(self._h, channel, TAPS[name], None, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(lib.fmrx_channels_read_tap(self._h, channel, TAPS[name], out.ctypes.data, C.byref(n)))
        return out

    def demod_layout(self):
        """(device address of channel 0's discriminator row of the last call, pitch in floats, IF samples per row): the input
        of RdsBank.process_dev on the same stream.  Not for the fused mono bank of modes 0/1 (FmrxError)."""
        ptr, pitch, n_if = _vp(), _sz(0), _sz(0)
        _check(lib.fmrx_channels_demod_layout(self._h, C.byref(ptr), C.byref(pitch), C.byref(n_if)))
        return ptr.value, pitch.value, n_if.value

    def load_dev(self, d_iq_ptr, stream=None):
        """Device-resident [n_channels, block_bytes] blocks -> the channels' slots (async on `stream`)."""
        _check(lib.fmrx_channels_load_dev(self._h, d_iq_ptr, stream))

    def process_dev(self, d_audio_ptr=None, d_pcm_ptr=None, wrap=True, stream=None):
        _check(lib.fmrx_channels_process_dev(self._h, d_audio_ptr, d_pcm_ptr, PCM_WRAP if wrap else PCM_SATURATE, stream))


# --------------------------------------------------------------------------
# RDS path: the model's names (model/fmSupportLib.py), float64
# --------------------------------------------------------------------------
RDS_TAPS = {"channel": 0, "carrier": 1, "pll_i": 2, "pll_q": 3, "resampled_i": 4, "rrc_i": 5, "rrc_q": 6, "pll_state": 7}


def rdsBandPass(N_taps, Fs, Fb, Fe) -> np.ndarray:
    """fmSupportLib.py:358 bandPass (Python argument order), float64."""
    h = np.zeros(N_taps)
    _check(lib.fmrx_rds_band_pass(N_taps, Fs, Fb, Fe, h))
    return h


def rdsImpResponse(N_taps, Fs, Fc) -> np.ndarray:
    h = np.zeros(N_taps)
    _check(lib.fmrx_rds_imp_response(N_taps, Fs, Fc, h))
    return h


def impulseResponseRootRaisedCosine(Fs, N_taps) -> np.ndarray:
    h = np.zeros(N_taps)
    _check(lib.fmrx_rds_rrc(Fs, N_taps, h))
    return h


def CDR(input1, rds_SPS, to_pass_on_state, block_count):
    """fmSupportLib.py:103 CDR -> (Manchester-decoded bits, [pair, next_start, size])."""
    x = np.ascontiguousarray(input1, np.float64)
    st = np.array([to_pass_on_state[0][0], to_pass_on_state[0][1], to_pass_on_state[1], to_pass_on_state[2]], np.float64)
    bits = np.zeros(len(x) // max(int(rds_SPS), 1) + 4, np.uint8)
    n = _sz(0)
    _check(lib.fmrx_rds_cdr(x, len(x), rds_SPS, block_count, st, bits, C.byref(n)))
    return bits[:n.value].astype(np.float64), [st[:2].copy(), int(st[2]), int(st[3])]


def diff_decoding(manch_data) -> np.ndarray:
    b = np.ascontiguousarray(manch_data, np.uint8)
    out = np.zeros(len(b), np.uint8)
    _check(lib.fmrx_rds_diff_decode(b, len(b), out))
    return out.astype(np.float64)


def framesync(diff_data):
    b = np.ascontiguousarray(diff_data, np.uint8)
    off, idx = C.create_string_buffer(8), _sz(0)
    _check(lib.fmrx_rds_frame_sync(b, len(b), off, C.byref(idx)))
    return off.value.decode(), idx.value


class Rds(_Handle):
    """The RDS chain of model/fmMonoBlock.py:238-296 on fm_demod blocks (fmrx_rds_*): the device chain of RdsBank with one channel,
    any block of up to max_block samples per call, bits recovered on the host."""
    _destroy = "fmrx_rds_destroy"

    def __init__(self, mode=0, max_block=9600, device=0, params: RdsParams | None = None):
        self.params = params if params is not None else RdsParams()
        if params is None:
            _check(lib.fmrx_rds_mode_params(mode, C.byref(self.params)))
        self._h = _vp()
        _check(lib.fmrx_rds_create(C.byref(self._h), C.byref(self.params), max_block, device))

    def reset(self):
        _check(lib.fmrx_rds_reset(self._h))

    def process(self, fm_demod):
        x = _f32(fm_demod)
        no = lib.fmrx_rds_n_out(self._h, len(x))
        yi, yq = np.zeros(no), np.zeros(no)
        bits, nb, off = np.zeros(no // max(self.params.sps, 1) + 4, np.uint8), _sz(0), C.create_string_buffer(8)
        _check(lib.fmrx_rds_process(self._h, x, len(x), yi.ctypes.data, yq.ctypes.data, bits.ctypes.data, C.byref(nb), off))
        return {"rrc_i": yi, "rrc_q": yq, "diff_bits": bits[:nb.value].copy(), "offset_type": off.value.decode()}

    def process_dev(self, d_demod_ptr, n, stream=None):
        _check(lib.fmrx_rds_process_dev(self._h, d_demod_ptr, n, stream))

    def read_tap(self, name) -> np.ndarray:
        n = _sz(0)
        _check(lib.fmrx_rds_read_tap(self._h, RDS_TAPS[name], None, C.byref(n)))
        out = np.zeros(n.value)
        _check(lib.fmrx_rds_read_tap(self._h, RDS_TAPS[name], out.ctypes.data, C.byref(n)))
        return out


class RdsBank(_Handle):
    """The RDS chain of N channels per device call (fmrx_rds_bank_*), bits recovered on the device.  An Rds handle runs the same
    chain with one channel, so per channel this is, bit for bit, what an Rds handle reports for the same discriminator stream.
    block: IF samples per channel and call (9600 = the receiver banks' block_bytes 192000)."""
    _destroy = "fmrx_rds_bank_destroy"

    def __init__(self, mode=0, n_channels=1, block=9600, device=0, params: RdsParams | None = None):
        self.params = params if params is not None else RdsParams()
        if params is None:
            _check(lib.fmrx_rds_mode_params(mode, C.byref(self.params)))
        self.n_channels, self.block = int(n_channels), int(block)
        self._h = _vp()
        _check(lib.fmrx_rds_bank_create(C.byref(self._h), C.byref(self.params), self.n_channels, self.block, device))
        self.n_out = lib.fmrx_rds_bank_n_out(self._h)
        self.max_bits = lib.fmrx_rds_bank_max_bits(self._h)

    def reset(self, channel=-1):
        _check(lib.fmrx_rds_bank_reset(self._h, channel))

    def _outputs(self, want_rrc=True):
        n = self.n_channels
        yi = np.zeros((n, self.n_out)) if want_rrc else None
        yq = np.zeros((n, self.n_out)) if want_rrc else None
        bits, nb, off = np.zeros((n, self.max_bits), np.uint8), np.zeros(n, np.uint64), C.create_string_buffer(8 * n)
        return yi, yq, bits, nb, off

    def _result(self, yi, yq, bits, nb, off):
        raw = off.raw
        return {"rrc_i": list(yi) if yi is not None else None, "rrc_q": list(yq) if yq is not None else None,
                "diff_bits": [bits[c, :int(nb[c])].copy() for c in range(self.n_channels)],
                "offset_type": [raw[8 * c:8 * c + 8].split(b"\0", 1)[0].decode() for c in range(self.n_channels)]}

    def process(self, demod):
        """demod: [n_channels, block] (host) -> dict(rrc_i, rrc_q, diff_bits: per-channel lists of arrays, offset_type: list of str)."""
        x = _f32(demod).reshape(self.n_channels, self.block)
        out = self._outputs()
        yi, yq, bits, nb, off = out
        _check(lib.fmrx_rds_bank_process(self._h, x.reshape(-1), yi.ctypes.data, yq.ctypes.data, bits.ctypes.data, nb.ctypes.data, off))
        return self._result(*out)

    def process_dev(self, d_demod_ptr, pitch, stream=None):
        """Device rows: channel c's block at d_demod_ptr + c*pitch floats (Channels.demod_layout()); async on `stream`."""
        _check(lib.fmrx_rds_bank_process_dev(self._h, d_demod_ptr, pitch, stream))

    def collect(self, want_rrc=True):
        """Waits for the last process_dev -> the same dict as process()."""
        out = self._outputs(want_rrc)
        yi, yq, bits, nb, off = out
        _check(lib.fmrx_rds_bank_collect(self._h, yi.ctypes.data if want_rrc else None, yq.ctypes.data if want_rrc else None,
                                         bits.ctypes.data, nb.ctypes.data, off))
        return self._result(*out)

    def set_stations(self, on=True, max_burst=0, ext=False):
        """A station decoder per channel on the device (off by default); only before the first call or right after reset().
        max_burst: burst error correction of blocks that fail while sync is held, 0 (off) .. 5; 2 is recommended: it repairs
        one wrong chip pair per block and takes 5 % of random words for blocks (5: 36 %).  ext=True keeps an extension record
        per channel (stations_ext).  With neither, the bank runs exactly what it ran before these options existed."""
        _check(lib.fmrx_rds_bank_set_stations(self._h, 1 if on else 0))
        if on and (max_burst or ext):
            _check(lib.fmrx_rds_bank_set_station_options(self._h, int(max_burst), 1 if ext else 0))
        self.max_groups = lib.fmrx_rds_bank_max_groups(self._h)

    def stations(self, raw=False):
        """Waits for the last process_dev -> (stations: list of dicts, groups: per channel the RDS_GROUP_DTYPE records of the last
        call).  raw=True: the station records as an RDS_STATION_DTYPE array [n_channels] instead of dicts."""
        n, mg = self.n_channels, lib.fmrx_rds_bank_max_groups(self._h)
        st = np.zeros(n, RDS_STATION_DTYPE)
        g = np.zeros((n, mg), RDS_GROUP_DTYPE)
        ng = np.zeros(n, np.uint64)
        _check(lib.fmrx_rds_bank_stations(self._h, st.ctypes.data, g.ctypes.data, ng.ctypes.data))
        groups = [g[c, :int(ng[c])].copy() for c in range(n)]
        return (st if raw else [rds_station_dict(r) for r in st]), groups

    def stations_ext(self, raw=False):
        """Waits for the last process_dev -> every channel's extension record (set_stations(ext=True)) as a list of
        rds_station_ext_dict; raw=True: as an RDS_STATION_EXT_DTYPE array [n_channels]."""
        x = np.zeros(self.n_channels, RDS_STATION_EXT_DTYPE)
        _check(lib.fmrx_rds_bank_stations_ext(self._h, x.ctypes.data))
        return x if raw else [rds_station_ext_dict(r) for r in x]

    def read_tap(self, channel, name) -> np.ndarray:
        n = _sz(0)
        _check(lib.fmrx_rds_bank_read_tap(self._h, channel, RDS_TAPS[name], None, C.byref(n)))
        out = np.zeros(n.value)
        _check(lib.fmrx_rds_bank_read_tap(self._h, channel, RDS_TAPS[name], out.ctypes.data, C.byref(n)))
        return out


# fmrx_rds_station / fmrx_rds_group (include/fmrx.h): 96 and 16 bytes, no padding
RDS_STATION_DTYPE = np.dtype([("pi", "<u2"), ("pty", "u1"), ("tp", "u1"), ("ta", "u1"), ("ms", "u1"), ("synced", "u1"), ("seen", "u1"),
                              ("ps_mask", "u1"), ("rt_ab", "u1"), ("rt_mask", "<u2"), ("blocks", "<u4"), ("good_blocks", "<u4"),
                              ("groups", "<u4"), ("ps", "u1", (8,)), ("rt", "u1", (64,))])
RDS_GROUP_DTYPE = np.dtype([("block", "<u2", (4,)), ("ok_mask", "u1"), ("reserved", "u1", (3,)), ("bit_index", "<u4")])
assert RDS_STATION_DTYPE.itemsize == 96 and RDS_GROUP_DTYPE.itemsize == 16
# fmrx_rds_station_ext: 128 bytes, no padding
RDS_STATION_EXT_DTYPE = np.dtype([("corrected_blocks", "<u4"), ("burst_hist", "<u4", (5,)), ("sync_losses", "<u4"), ("group_types", "<u4"),
                                  ("af_bits", "<u4", (8,)), ("ct_mjd", "<u4"), ("ct_bit_index", "<u4"), ("ct_count", "<u4"),
                                  ("ptyn", "u1", (8,)), ("pin", "<u2"), ("lang", "<u2"), ("ecc", "u1"), ("ext_seen", "u1"),
                                  ("max_burst", "u1"), ("di", "u1"), ("di_mask", "u1"), ("af_announced", "u1"), ("ct_hour", "u1"),
                                  ("ct_minute", "u1"), ("ct_offset", "u1"), ("ptyn_mask", "u1"), ("ptyn_ab", "u1"),
                                  ("reserved", "u1", (29,))])
assert RDS_STATION_EXT_DTYPE.itemsize == 128


def rds_station_dict(rec) -> dict:
    """One fmrx_rds_station record (an element of an RDS_STATION_DTYPE array) -> dict; ps and rt as str (latin-1: the RDS
    character table agrees with ASCII for the letters, digits and punctuation)."""
    d = {k: int(rec[k]) for k in ("pi", "pty", "tp", "ta", "ms", "seen", "ps_mask", "rt_ab", "rt_mask", "blocks", "good_blocks", "groups")}
    d["synced"] = bool(rec["synced"])
    d["ps"] = bytes(rec["ps"]).decode("latin-1")
    d["rt"] = bytes(rec["rt"]).decode("latin-1")
    return d


def rds_station_ext_dict(rec) -> dict:
    """One fmrx_rds_station_ext record (an element of an RDS_STATION_EXT_DTYPE array) -> dict.  af: the alternative
    frequencies as a sorted list of MHz; ct: None, or the last clock time as dict(mjd, hour, minute, offset_minutes (signed),
    bit_index); group_types: such as ["0A", "2A", "4A"]; ecc / lang / pin: None until received; ptyn as str."""
    d = {k: int(rec[k]) for k in ("corrected_blocks", "sync_losses", "max_burst", "di", "di_mask", "af_announced", "ct_count",
                                  "ptyn_mask", "ptyn_ab")}
    d["burst_hist"] = [int(v) for v in rec["burst_hist"]]
    gt = int(rec["group_types"])
    d["group_types"] = [f"{k >> 1}{'AB'[k & 1]}" for k in range(32) if (gt >> k) & 1]
    af = [int(w) for w in rec["af_bits"]]
    d["af"] = [round(87.5 + 0.1 * c, 1) for c in range(1, 205) if (af[c >> 5] >> (c & 31)) & 1]
    seen = int(rec["ext_seen"])
    d["ecc"] = int(rec["ecc"]) if seen & 1 else None
    d["lang"] = int(rec["lang"]) if seen & 2 else None
    d["pin"] = int(rec["pin"]) if seen & 4 else None
    off = int(rec["ct_offset"])
    d["ct"] = None if d["ct_count"] == 0 else {"mjd": int(rec["ct_mjd"]), "hour": int(rec["ct_hour"]), "minute": int(rec["ct_minute"]),
                                               "offset_minutes": (-30 if off & 32 else 30) * (off & 31), "bit_index": int(rec["ct_bit_index"])}
    d["ptyn"] = bytes(rec["ptyn"]).decode("latin-1")
    return d


def rds_block_correct(word26: int, offset: int, max_burst: int):
    """fmrx_rds_block_correct: one 26-bit block against offset 0 A, 1 B, 2 C, 3 C', 4 D -> (status 0 clean / 1 corrected /
    2 uncorrectable, information word, burst length)."""
    info, n = C.c_uint16(0), _int(0)
    rc = lib.fmrx_rds_block_correct(word26, offset, max_burst, C.byref(info), C.byref(n))
    if rc < 0:
        raise FmrxError(EINVAL, "rds_block_correct: bad argument")
    return rc, info.value, n.value


class RdsStationDecoder(_Handle):
    """The RDS station decoder on the host (fmrx_rds_station_*): PI, PTY, PS and RadioText from the in-phase matched-filter rows
    an Rds handle returns (feed_rrc), or from differentially decoded bits (feed_bits).  State carries across feeds.  Each feed
    returns (station dict, the groups it completed as an RDS_GROUP_DTYPE array); .record holds the raw station record and .ext
    the raw extension record (RDS_STATION_EXT_DTYPE [1]; rds_station_ext_dict).  max_burst: burst error correction, 0 (off)
    .. 5; 2 is recommended (one wrong chip pair per block is repaired; 5 % of random words pass for blocks, at 5: 36 %)."""
    _destroy = "fmrx_rds_station_destroy"

    def __init__(self, mode=0, sps: int | None = None, max_burst=0):
        if sps is None:
            p = RdsParams()
            _check(lib.fmrx_rds_mode_params(mode, C.byref(p)))
            sps = p.sps
        self.sps = int(sps)
        self._h = _vp()
        _check(lib.fmrx_rds_station_create(C.byref(self._h), self.sps))
        self.max_burst = int(max_burst)
        if self.max_burst:
            try:
                _check(lib.fmrx_rds_station_set_correction(self._h, self.max_burst))
            except FmrxError:
                self.close()
                raise
        self.record = np.zeros(1, RDS_STATION_DTYPE)

    @property
    def ext(self):
        x = np.zeros(1, RDS_STATION_EXT_DTYPE)
        _check(lib.fmrx_rds_station_ext_get(self._h, x.ctypes.data))
        return x

    def reset(self):
        _check(lib.fmrx_rds_station_reset(self._h))

    def _feed(self, fn, data, max_g):
        g, n = np.zeros(max_g, RDS_GROUP_DTYPE), _sz(0)
        rec = np.zeros(1, RDS_STATION_DTYPE)
        _check(fn(self._h, data.ctypes.data, len(data), g.ctypes.data, max_g, C.byref(n), rec.ctypes.data))
        self.record = rec
        return rds_station_dict(rec[0]), g[:n.value].copy()

    def feed_rrc(self, row):
        x = np.ascontiguousarray(row, np.float64)
        return self._feed(lib.fmrx_rds_station_feed_rrc, x, lib.fmrx_rds_station_max_groups(self._h, len(x)))

    def feed_bits(self, bits):
        b = np.ascontiguousarray(np.asarray(bits) != 0, np.uint8)
        return self._feed(lib.fmrx_rds_station_feed_bits, b, 2 * (len(b) // 26 + 1))


# --------------------------------------------------------------------------
# Wideband tuner: one wide capture -> the input slots of a receiver bank
# --------------------------------------------------------------------------
def tunerLowPass(Fs_w, R, T) -> np.ndarray:
    """The default prototype filter of a Tuner: impulseResponseLPF(Fs_w, Fc, T) with Fc half-way between what has to pass
    and what has to stop.  Pass band: the +-128 kHz an FM channel occupies (75 kHz deviation + the 53 kHz multiplex).  Stop
    band: from rf_Fs - 100 kHz (rf_Fs = Fs_w / R), the lowest offset whose alias after decimation lands inside the bank's own
    100 kHz front-end low-pass.  Fc = (128 kHz + rf_Fs - 100 kHz) / 2: half-way, so the Hann-windowed design's transition
    (about 2 Fs_w / T to either side) clears both edges from T = 8 R on: at T = 8 R the response is within 0.03 dB of its DC
    gain at 128 kHz and below -54 dB from the stop-band edge to Fs_w / 2, for rf_Fs = 2.4 / 1.44 / 0.96 MS/s and R = 4 ... 20."""
    rf_Fs = float(Fs_w) / int(R)
    return impulseResponseLPF(float(Fs_w), 0.5 * (128e3 + rf_Fs - 100e3), int(T))


def tunerLowPassRational(Fs_w, U, D, T) -> np.ndarray:
    """The default prototype filter of Tuner.rational: tunerLowPass's rule at the upsampled rate U * Fs_w, with the gain U
    that makes the pass band unity after zero-stuffing:  U * impulseResponseLPF(U * Fs_w, Fc, T),  rf_Fs = Fs_w * U / D,
    Fc = (128 kHz + rf_Fs - 100 kHz) / 2.  At T = 8 D (Tp = 8 D / U taps per phase, the transition the integer tuner has at
    T = 8 R), the float32 taps' response at 128 kHz against DC and the largest response from rf_Fs - 100 kHz to U Fs_w / 2:
        6/25, 3/25 (10, 20 -> 2.4 MS/s), 24/125 (12.5 -> 2.4), 3/10, 3/20 (8, 16 -> 2.4):  within 0.011 dB, below -62.4 dB
        18/125 (10 -> 1.44 MS/s):                                                          -0.023 dB, -61.2 dB
        12/125 (10 -> 0.96 MS/s, 25 -> 2.4 MS/s):                                          -0.032 dB, -54.9 dB"""
    rf_Fs = float(Fs_w) * int(U) / int(D)
    return (np.float32(U) * impulseResponseLPF(int(U) * float(Fs_w), 0.5 * (128e3 + rf_Fs - 100e3), int(T))).astype(np.float32)


TUNER_FORMATS = {"u8": 0, "s8": 1, "s16": 2}                       # FMRX_TUNER_U8 / _S8 / _S16
_TUNER_DTYPES = {"u8": np.uint8, "s8": np.int8, "s16": np.int16}


class Tuner(_Handle):
    """N channels of one wide I/Q capture (Fs_w = R * rf_Fs), each mixed to its own centre offset, low-pass filtered by
    the prototype h and decimated by R, as u8 I/Q rows: the input of a receiver bank (fmrx_tuner_*; exact integer
    arithmetic).  tuner.process_dev(d_wide, n_wide, *bank.input_layout(), stream) followed by
    bank.process_dev(..., stream=stream) runs capture -> audio without the samples leaving the device.
    fmt: the capture's format, "u8" (interleaved unsigned bytes), "s8" (int8) or "s16" (int16, 4 bytes per complex sample;
    a device with 12 or 14 bits in the low end of the short takes a gain of 16 or 4)."""
    _destroy = "fmrx_tuner_destroy"

    def __init__(self, R, h, n_channels, max_wide_samples, device=0, fmt="u8"):
        self._open(lib.fmrx_tuner_create_ex, (int(R),), 1, int(R), h, n_channels, max_wide_samples, device, fmt)

    @classmethod
    def rational(cls, U, D, h, n_channels, max_wide_samples, device=0, fmt="u8"):
        """A Tuner at rf_Fs = Fs_w * U / D (gcd 1, 1 <= U <= 32, 2 U <= D <= 512): h is the prototype low-pass at U * Fs_w
        (tunerLowPassRational), calls take a multiple of D wide samples and give n_wide * U / D outputs per channel
        (fmrx_tuner_create_rational).  .U and .D hold the ratio; .R is D for U = 1, else None."""
        self = cls.__new__(cls)
        self._open(lib.fmrx_tuner_create_rational, (int(U), int(D)), int(U), int(D), h, n_channels, max_wide_samples, device, fmt)
        return self

    def _open(self, create, rate_args, U, D, h, n_channels, max_wide_samples, device, fmt):
        if fmt not in TUNER_FORMATS:
            raise ValueError(f"Tuner: fmt {fmt!r}: one of {', '.join(TUNER_FORMATS)}")
        self.U, self.D, self.R = U, D, D if U == 1 else None
        self.n_channels, self.max_wide_samples, self.fmt = int(n_channels), int(max_wide_samples), fmt
        self.h = _f32(h)
        self._h = _vp()
        _check(create(C.byref(self._h), *rate_args, self.h, len(self.h), self.n_channels, self.max_wide_samples, TUNER_FORMATS[fmt], device))
        self.sample_bytes = int(lib.fmrx_tuner_sample_bytes(self._h))       # per complex wide sample: 2, 2 or 4

    def ratio(self):
        """(U, D) as the handle reports it: (1, R) for an integer tuner"""
        u, d = _int(0), _int(0)
        _check(lib.fmrx_tuner_ratio(self._h, C.byref(u), C.byref(d)))
        return u.value, d.value

    @staticmethod
    def design_rational(h, U, Fs_w, f_c, gain=1.0):
        """Host only: (frequency word, scale exponent s, re int16[U * Tp], im int16[U * Tp]) of one channel of a rational
        tuner, phase-major (tap j of phase p at p * Tp + j, Tp = ceil(len(h) / U))."""
        h = _f32(h)
        U = int(U)
        n = U * (-(-len(h) // U)) if 1 <= U <= 32 else len(h)             # another U: the library rejects it
        w, s = C.c_uint32(0), _int(0)
        re, im = np.zeros(n, np.int16), np.zeros(n, np.int16)
        _check(lib.fmrx_tuner_design_rational(h, len(h), U, Fs_w, f_c, gain, C.byref(w), C.byref(s), re, im))
        return w.value, s.value, re, im

    @staticmethod
    def design(h, Fs_w, f_c, gain=1.0):
        """Host only: (frequency word, scale exponent s, re int16[T], im int16[T]) of one channel of an integer tuner."""
        return Tuner.design_rational(h, 1, Fs_w, f_c, gain)

    @staticmethod
    def table():
        """Host only: the rotation table (cos, sin) as int16[4096] each."""
        n = _sz(0)
        _check(lib.fmrx_tuner_table(None, None, C.byref(n)))
        c, s = np.zeros(n.value, np.int16), np.zeros(n.value, np.int16)
        _check(lib.fmrx_tuner_table(c.ctypes.data, s.ctypes.data, C.byref(n)))
        return c, s

    def reset(self):
        _check(lib.fmrx_tuner_reset(self._h))

    def set_channel(self, channel, f_c_hz, Fs_w, gain=1.0):
        _check(lib.fmrx_tuner_set_channel(self._h, channel, f_c_hz, Fs_w, gain))

    def n_out_bytes(self, n_wide):
        return lib.fmrx_tuner_n_out_bytes(self._h, n_wide)

    def plan(self, n_wide):
        """For tests and diagnostics, host only: what a call of n_wide wide samples launches, as a dict of matrix, tiles, via_lds
        (bools and an int), lds_bytes, n_steps, steps_per_wg, grid_x, grid_y (fmrx_tuner_plan)."""
        p = TunerPlanInfo()
        _check(lib.fmrx_tuner_plan(self._h, int(n_wide), C.byref(p)))
        return {"matrix": bool(p.matrix), "tiles": p.tiles, "via_lds": bool(p.via_lds), "lds_bytes": p.lds_bytes, "n_steps": p.n_steps,
                "steps_per_wg": p.steps_per_wg, "grid_x": p.grid_x, "grid_y": p.grid_y}

    def process(self, wide):
        """wide: interleaved I,Q (host) as uint8 / int8 / int16 for fmt u8 / s8 / s16 (another dtype is a TypeError, never a
        conversion), a multiple of R (of D for a rational tuner) samples -> uint8 [n_channels, n_out_bytes(n_wide)]."""
        if self.fmt == "u8" and not isinstance(wide, np.ndarray):
            wide = _u8(wide)
        if not isinstance(wide, np.ndarray) or wide.dtype != _TUNER_DTYPES[self.fmt]:
            raise TypeError(f"Tuner.process: a {self.fmt} tuner takes a {np.dtype(_TUNER_DTYPES[self.fmt]).name} array, not {getattr(wide, 'dtype', type(wide).__name__)}")
        x = np.ascontiguousarray(wide).reshape(-1)
        n_wide = len(x) // 2
        out = np.zeros((self.n_channels, self.n_out_bytes(n_wide)), np.uint8)
        _check(lib.fmrx_tuner_process(self._h, x.ctypes.data, n_wide, out.reshape(-1)))
        return out

    def process_dev(self, d_wide_ptr, n_wide, d_out_first, pitch_bytes, stream=None):
        _check(lib.fmrx_tuner_process_dev(self._h, d_wide_ptr, n_wide, d_out_first, pitch_bytes, stream))

    def levels(self):
        """Of the last call, per channel: (output bytes that clamped, sum of (I-128)^2 + (Q-128)^2) as uint64 arrays."""
        cl, pw = np.zeros(self.n_channels, np.uint64), np.zeros(self.n_channels, np.uint64)
        _check(lib.fmrx_tuner_levels(self._h, cl.ctypes.data, pw.ctypes.data))
        return cl, pw


# --------------------------------------------------------------------------
# Signal meters: level, CNR, pilot, RDS, deviation of every channel of a bank
# --------------------------------------------------------------------------
METERS_SEGMENT = 1024
METER_DTYPE = np.dtype([("n_iq", "<u8"), ("sum_i", "<i8"), ("sum_q", "<i8"), ("m2", "<u8"), ("m4", "<u8"), ("clipped", "<u8"),
                        ("n_if", "<u8"), ("segments", "<u8"), ("sum_x", "<f8"), ("sum_x2", "<f8"), ("max_abs", "<f8"),
                        ("probe", "<f8", (8,))])                 # struct fmrx_meter
METER_LEVELS_DTYPE = np.dtype([(k, "<f8") for k in ("level_dbfs", "cnr_db", "clip_fraction", "dc_i", "dc_q", "freq_offset_hz",
                                                    "peak_dev_hz", "mpx_rms_hz", "pilot_dev_hz", "pilot_db", "rds_db")])   # struct fmrx_meter_levels
assert METER_DTYPE.itemsize == 152 and METER_LEVELS_DTYPE.itemsize == 88


def metersProbes() -> np.ndarray:
    """Host only: the probe frequencies in Hz (noise low, noise high, pilot, RDS low, RDS high)."""
    hz, n = np.zeros(8), _int(0)
    _check(lib.fmrx_meters_probes(hz, C.byref(n)))
    return hz[:n.value]


def metersTable(if_Fs):
    """Host only: the windowed tone table (re, im), float64 [5, 1024] each, as the device uses it."""
    re, im = np.zeros((5, METERS_SEGMENT)), np.zeros((5, METERS_SEGMENT))
    _check(lib.fmrx_meters_table(float(if_Fs), re.reshape(-1), im.reshape(-1)))
    return re, im


def metersDerive(if_Fs, rec) -> dict:
    """Host only: the levels (fmrx_meter_levels, as a dict) of one METER_DTYPE record."""
    r = np.array(rec, dtype=METER_DTYPE).reshape(1)
    out = np.zeros(1, METER_LEVELS_DTYPE)
    _check(lib.fmrx_meters_derive(float(if_Fs), r.ctypes.data, out.ctypes.data))
    return {k: float(out[0][k]) for k in METER_LEVELS_DTYPE.names}


class Meters(_Handle):
    """Per channel of a receiver bank and call: RF level, CNR and clipping of the input slot, and frequency offset,
    deviation, pilot and RDS levels of the discriminator row (fmrx_meters_*).  One pass over what
    the bank's call left on the device: meters = Meters.for_bank(bank); after bank.process_dev(..., stream=s),
    meters.process_bank(stream=s); recs = meters.collect(); meters.derive(recs[c])."""
    _destroy = "fmrx_meters_destroy"

    def __init__(self, if_Fs, n_channels=1, device=0):
        self.if_Fs, self.n_channels = float(if_Fs), int(n_channels)
        self._bank = None
        self._h = _vp()
        _check(lib.fmrx_meters_create(C.byref(self._h), self.if_Fs, self.n_channels, device))

    @classmethod
    def for_bank(cls, bank):
        """The meters of a Channels bank, on the bank's device; process_bank() then passes the bank's own layouts (no
        discriminator rows where the bank keeps none: the fused mono bank of modes 0/1)."""
        m = cls(bank.params.if_Fs, bank.n_channels, bank.device)
        m._bank = bank
        return m

    def process_dev(self, d_iq_first, iq_pitch_bytes, n_iq_bytes, d_demod_row0, demod_pitch, n_if, stream=None):
        """Device rows as Channels.input_layout() / demod_layout() return them; either pointer may be None."""
        _check(lib.fmrx_meters_process_dev(self._h, d_iq_first, iq_pitch_bytes, n_iq_bytes, d_demod_row0, demod_pitch, n_if, stream))

    def process_bank(self, stream=None):
        """process_dev on the layouts of the bank given to for_bank (asked again at every call: the rows' address is the last call's)."""
        bank = self._bank
        first, pitch = bank.input_layout()
        try:
            rows, row_pitch, n_if = bank.demod_layout()
        except FmrxError as e:
            if e.code != EINVAL:     # EINVAL: this bank keeps no rows; anything else is a failure of its own
                raise
            rows, row_pitch, n_if = None, 0, 0
        self.process_dev(first, pitch, bank.block_bytes, rows, row_pitch, n_if, stream)

    def collect(self) -> np.ndarray:
        """Waits for the last call; METER_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, METER_DTYPE)
        _check(lib.fmrx_meters_collect(self._h, out.ctypes.data))
        return out

    def process(self, iq=None, demod=None) -> np.ndarray:
        """Host rows: iq uint8 [n_channels, n_iq_bytes] and / or demod float32 [n_channels, n_if] -> METER_DTYPE [n_channels]."""
        iq = None if iq is None else _u8(iq).reshape(self.n_channels, -1)
        x = None if demod is None else _f32(demod).reshape(self.n_channels, -1)
        out = np.zeros(self.n_channels, METER_DTYPE)
        _check(lib.fmrx_meters_process(self._h, None if iq is None else iq.ctypes.data, 0 if iq is None else iq.shape[1],
                                       0 if iq is None else iq.shape[1], None if x is None else x.ctypes.data,
                                       0 if x is None else x.shape[1], 0 if x is None else x.shape[1], out.ctypes.data))
        return out

    def derive(self, rec) -> dict:
        return metersDerive(self.if_Fs, rec)


# --------------------------------------------------------------------------
# What the stages behind the meters share
# --------------------------------------------------------------------------
def _params_init(self, defaults, kw):
    """The keyword constructor of BlendParams and HighCutParams: the library's defaults, then single fields by name."""
    C.Structure.__init__(self)
    _check(defaults(C.byref(self)))
    kinds = dict(self._fields_)
    for k, v in kw.items():
        if k not in kinds:
            raise TypeError(f"{type(self).__name__} has no field {k!r}")
        setattr(self, k, int(v) if kinds[k] is C.c_int32 else float(v))


class _MeterStage(_Handle):
    """What Blend, HighCut and Leveller share: a handle behind a meters handle on a bank's audio (csrc/meter_stage.hpp).  A
    subclass names its fmrx_<_prefix>_* functions, its status dtype and the dtype of the records its host call reads, and creates
    self._h."""
    _status_dtype = None
    _rec_dtype = METER_DTYPE

    def reset(self, channel=-1):
        self._call("reset", channel)

    def process_dev(self, meters, d_in, d_out=None, d_pcm=None, stream=None, wrap=True):
        """Device rows [n_channels, audio_channels, n_audio] float32 -> d_out (may be d_in) and / or d_pcm [n_channels, n_audio,
        audio_channels] int16, asynchronous on `stream` behind meters.process_dev on the same stream."""
        self._call("process_dev", meters._h, d_in, d_out, d_pcm, PCM_WRAP if wrap else PCM_SATURATE, stream)

    def process_bank(self, d_in, d_out=None, d_pcm=None, stream=None, wrap=True):
        """process_dev with the Meters given to for_bank."""
        self.process_dev(self._meters, d_in, d_out, d_pcm, stream, wrap)

    def process(self, recs, audio, want_f32=True, want_pcm=True, wrap=True, in_place=False):
        """Host records [n_channels] (METER_DTYPE; the leveller: AUDIO_METER_DTYPE, AudioMeters.collect's) and host rows float32
        [n_channels, audio_channels, n_audio], synchronous -> dict(audio=..., pcm16=[n_channels, n_audio, audio_channels]);
        in_place: the call writes over its input (audio is then an array of its own, never the caller's; the leveller refuses
        it, its output must not overlap its input).  The rows keep their host address modulo 16 on the device."""
        r = np.ascontiguousarray(recs, dtype=self._rec_dtype).reshape(self.n_channels)
        shape = (self.n_channels, self.audio_channels, self.n_audio)
        x = _f32(audio).reshape(shape)
        f = s = None
        if want_f32:
            if in_place:
                pad = np.zeros(x.size + 4, np.float32)           # a copy at the caller's address modulo 16
                o = ((x.ctypes.data - pad.ctypes.data) % 16) // 4
                f = pad[o:o + x.size].reshape(shape)
                f[...] = x
                x = f
            else:
                f = np.zeros(shape, np.float32)
        if want_pcm:
            s = np.zeros((self.n_channels, self.n_audio, self.audio_channels), np.int16)
        self._call("process", r.ctypes.data, x.ctypes.data, None if f is None else f.ctypes.data, None if s is None else s.ctypes.data,
                   PCM_WRAP if wrap else PCM_SATURATE)
        return {"audio": f, "pcm16": s}

    def status(self) -> np.ndarray:
        """Waits for the last call; the stage's status records (BLEND_STATUS_DTYPE, HIGHCUT_STATUS_DTYPE) [n_channels]."""
        out = np.zeros(self.n_channels, self._status_dtype)
        self._call("status_get", out.ctypes.data)
        return out


# --------------------------------------------------------------------------
# Stereo blend and soft mute behind a bank, driven by the meters
# --------------------------------------------------------------------------
class BlendParams(C.Structure):
    """struct fmrx_blend_params: thresholds in dB, mute_floor in [0, 1], attack / release per call in (0, 1].  BlendParams()
    holds the library's defaults; keyword arguments replace single fields."""
    _fields_ = [(k, C.c_double) for k in ("pilot_on", "pilot_off", "blend_lo", "blend_hi", "mute_lo", "mute_hi", "mute_floor",
                                          "attack", "release")]

    def __init__(self, **kw):
        _params_init(self, lib.fmrx_blend_defaults, kw)


BLEND_STATUS_DTYPE = np.dtype([("pilot_db", "<f8"), ("quiet_db", "<f8"), ("sep_target", "<f8"), ("gain_target", "<f8"), ("sep", "<f8"),
                               ("gain", "<f8"), ("mono0", "<f4"), ("gain0", "<f4"), ("mono1", "<f4"), ("gain1", "<f4"), ("lamp", "<u4"),
                               ("reserved", "<u4"), ("calls", "<u8")])                 # struct fmrx_blend_status
assert BLEND_STATUS_DTYPE.itemsize == 80 and C.sizeof(BlendParams) == 72
_sig("fmrx_blend_defaults", [C.POINTER(BlendParams)])
_sig("fmrx_blend_control", [C.POINTER(BlendParams), _dbl, _vp, _vp])
_sig("fmrx_blend_create", [C.POINTER(_vp), C.POINTER(BlendParams), _dbl, _int, _int, _sz, _int])
_sig("fmrx_blend_destroy", [_vp])
_sig("fmrx_blend_reset", [_vp, _int])
_sig("fmrx_blend_process_dev", [_vp, _vp, _vp, _vp, _vp, _int, _vp])
_sig("fmrx_blend_process", [_vp, _vp, _vp, _vp, _vp, _int])
_sig("fmrx_blend_status_get", [_vp, _vp])


def blendControl(params, if_Fs, rec, state=None) -> np.ndarray:
    """Host only: one channel's control step (fmrx_blend_control) on one METER_DTYPE record; state: the BLEND_STATUS_DTYPE
    record the last step returned (None or zeros: a fresh channel) -> the new one."""
    r = np.array(rec, dtype=METER_DTYPE).reshape(1)
    st = np.zeros(1, BLEND_STATUS_DTYPE) if state is None else np.array(state, dtype=BLEND_STATUS_DTYPE).reshape(1).copy()
    p = params if params is not None else BlendParams()
    _check(lib.fmrx_blend_control(C.byref(p), float(if_Fs), r.ctypes.data, st.ctypes.data))
    return st[0]


class Blend(_MeterStage):
    """Stereo lamp, blend towards mono and soft mute per channel of a receiver bank, decided from the meters' pilot and noise
    powers of the same call and applied to the bank's audio (fmrx_blend_*).  blend = Blend.for_bank(bank,
    meters); after bank.process_dev(d_audio, ..., stream=s) and meters.process_bank(stream=s):
    blend.process_bank(d_audio, d_out, d_pcm, stream=s); blend.status()."""

    _prefix, _status_dtype = "blend", BLEND_STATUS_DTYPE

    def __init__(self, if_Fs, n_channels=1, audio_channels=2, n_audio=1920, params: BlendParams | None = None, device=0):
        self.if_Fs, self.n_channels, self.audio_channels, self.n_audio = float(if_Fs), int(n_channels), int(audio_channels), int(n_audio)
        self.params = params if params is not None else BlendParams()
        self._meters = None
        self._h = _vp()
        _check(lib.fmrx_blend_create(C.byref(self._h), C.byref(self.params), self.if_Fs, self.n_channels, self.audio_channels,
                                     self.n_audio, device))

    @classmethod
    def for_bank(cls, bank, meters, params: BlendParams | None = None):
        """The blend stage of a Channels bank and of the Meters made for it, on the bank's device."""
        b = cls(bank.params.if_Fs, bank.n_channels, bank.audio_channels, bank.n_audio, params, bank.device)
        b._meters = meters
        return b

    @staticmethod
    def coef(tau_s, call_s) -> float:
        """The attack / release coefficient of a time constant tau_s at one call every call_s seconds: 1 - exp(-call_s / tau_s)."""
        return 1.0 - float(np.exp(-float(call_s) / float(tau_s)))


# --------------------------------------------------------------------------
# Variable high-cut behind the blend (or a bank), driven by the meters
# --------------------------------------------------------------------------
class HighCutParams(C.Structure):
    """struct fmrx_highcut_params: fc_min in Hz, hc_lo / hc_hi in dB of quieting, cut_max in [0, 1], attack / release per call in
    (0, 1], warmup / segment the parallel walk's lane shape (-1 = built-in).  HighCutParams() holds the library's defaults;
    keyword arguments replace single fields."""
    _fields_ = [(k, C.c_double) for k in ("fc_min", "hc_lo", "hc_hi", "cut_max", "attack", "release")] + \
               [("warmup", C.c_int32), ("segment", C.c_int32)]

    def __init__(self, **kw):
        _params_init(self, lib.fmrx_highcut_defaults, kw)


HIGHCUT_STATUS_DTYPE = np.dtype([("quiet_db", "<f8"), ("open_target", "<f8"), ("open", "<f8"), ("p0", "<f4"), ("p1", "<f4"),
                                 ("calls", "<u8")])                                 # struct fmrx_highcut_status
assert HIGHCUT_STATUS_DTYPE.itemsize == 40 and C.sizeof(HighCutParams) == 56
_sig("fmrx_highcut_defaults", [C.POINTER(HighCutParams)])
_sig("fmrx_highcut_design", [_dbl, _dbl, C.POINTER(C.c_float)])
_sig("fmrx_highcut_control", [C.POINTER(HighCutParams), _dbl, _dbl, _vp, _vp])
_sig("fmrx_highcut_create", [C.POINTER(_vp), C.POINTER(HighCutParams), _dbl, _dbl, _int, _int, _sz, _int])
_sig("fmrx_highcut_destroy", [_vp])
_sig("fmrx_highcut_reset", [_vp, _int])
_sig("fmrx_highcut_set_force", [_vp, _int])
_sig("fmrx_highcut_process_dev", [_vp, _vp, _vp, _vp, _vp, _int, _vp])
_sig("fmrx_highcut_process", [_vp, _vp, _vp, _vp, _vp, _int])
_sig("fmrx_highcut_status_get", [_vp, _vp])
_sig("fmrx_highcut_diagnostics", [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])


def highCutDesign(fc_min, audio_Fs) -> np.float32:
    """Host only: the float32 pole at full cut, float32(exp(-2 pi fc_min / audio_Fs)); FmrxError where it exceeds 0.875."""
    p = C.c_float()
    _check(lib.fmrx_highcut_design(float(fc_min), float(audio_Fs), C.byref(p)))
    return np.float32(p.value)


def highCutControl(params, if_Fs, audio_Fs, rec, state=None) -> np.ndarray:
    """Host only: one channel's control step (fmrx_highcut_control) on one METER_DTYPE record; state: the HIGHCUT_STATUS_DTYPE
    record the last step returned (None or zeros: a fresh channel) -> the new one."""
    r = np.array(rec, dtype=METER_DTYPE).reshape(1)
    st = np.zeros(1, HIGHCUT_STATUS_DTYPE) if state is None else np.array(state, dtype=HIGHCUT_STATUS_DTYPE).reshape(1).copy()
    p = params if params is not None else HighCutParams()
    _check(lib.fmrx_highcut_control(C.byref(p), float(if_Fs), float(audio_Fs), r.ctypes.data, st.ctypes.data))
    return st[0]


class HighCut(_MeterStage):
    """A one-pole low-pass per audio row of a receiver bank whose corner follows the channel's quieting, decided from the
    meters' noise powers of the same call (fmrx_highcut_*).  hc = HighCut.for_bank(bank, meters); after
    bank.process_dev, meters.process_bank and (where there is one) blend.process_bank on stream s:
    hc.process_bank(d_audio, d_out, d_pcm, stream=s); hc.status(); hc.diagnostics()."""

    _prefix, _status_dtype = "highcut", HIGHCUT_STATUS_DTYPE

    def __init__(self, if_Fs, audio_Fs=48000.0, n_channels=1, audio_channels=2, n_audio=1920, params: HighCutParams | None = None, device=0):
        self.if_Fs, self.audio_Fs = float(if_Fs), float(audio_Fs)
        self.n_channels, self.audio_channels, self.n_audio = int(n_channels), int(audio_channels), int(n_audio)
        self.params = params if params is not None else HighCutParams()
        self._meters = None
        self._h = _vp()
        _check(lib.fmrx_highcut_create(C.byref(self._h), C.byref(self.params), self.if_Fs, self.audio_Fs, self.n_channels,
                                       self.audio_channels, self.n_audio, device))

    @classmethod
    def for_bank(cls, bank, meters, params: HighCutParams | None = None):
        """The high-cut stage of a Channels bank and of the Meters made for it, on the bank's device."""
        h = cls(bank.params.if_Fs, bank.params.audio_Fs, bank.n_channels, bank.audio_channels, bank.n_audio, params, bank.device)
        h._meters = meters
        return h

    def force_serial(self, on=True):
        """Later calls walk their rows serially, one lane per row: the same bits, nothing counted in diagnostics()."""
        _check(lib.fmrx_highcut_set_force(self._h, int(bool(on))))

    def diagnostics(self) -> dict:
        """Waits for the last call; segments: the segment boundaries checked since create, missed: the segments walked again."""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        _check(lib.fmrx_highcut_diagnostics(self._h, C.byref(a), C.byref(b)))
        return {"segments": a.value, "missed": b.value}


# --------------------------------------------------------------------------
# Audio meters: peak, RMS, BS.1770 loudness, stereo image of every channel of a bank
# --------------------------------------------------------------------------
AUDIO_METER_DTYPE = np.dtype([("n", "<u8"), ("over", "<u8", (2,)), ("peak", "<f8", (2,)), ("sum_x", "<f8", (2,)), ("sum_x2", "<f8", (2,)),
                              ("sum_k2", "<f8", (2,)), ("sum_lr", "<f8"), ("bins_done", "<u8")])              # struct fmrx_audio_meter
AUDIO_METER_STATE_DTYPE = np.dtype([("z", "<f8", (2, 4)), ("bin_acc", "<f8", (2,)), ("bin_fill", "<u8")])    # struct fmrx_audio_meter_state
AUDIO_LEVELS_DTYPE = np.dtype([("peak_dbfs", "<f8", (2,)), ("rms_dbfs", "<f8", (2,)), ("dc", "<f8", (2,)), ("loudness_lkfs", "<f8"),
                               ("correlation", "<f8"), ("balance_db", "<f8"), ("over_fraction", "<f8")])     # struct fmrx_audio_levels
LOUDNESS_LEVELS_DTYPE = np.dtype([("momentary", "<f8"), ("short_term", "<f8"), ("integrated", "<f8"), ("blocks", "<u8"), ("full", "<u4"),
                                  ("reserved", "<u4")])                                                      # struct fmrx_loudness_levels
assert AUDIO_METER_DTYPE.itemsize == 104 and AUDIO_METER_STATE_DTYPE.itemsize == 88 and AUDIO_LEVELS_DTYPE.itemsize == 80
assert LOUDNESS_LEVELS_DTYPE.itemsize == 40
AUDIO_FULL_SCALE = 2.0    # the float value the PCM pack maps to 32 768
_sig("fmrx_audio_meters_design", [_dbl, _f64p])
_sig("fmrx_audio_meters_bin_len", [_dbl], _sz)
_sig("fmrx_audio_meters_max_bins", [_dbl, _sz], _sz)
_sig("fmrx_audio_meters_walk", [_dbl, _int, _vp, _sz, _sz, _vp, _vp, _vp, _sz])
_sig("fmrx_audio_meters_derive", [_vp, _int, _dbl, _vp])
_sig("fmrx_audio_meters_create", [C.POINTER(_vp), _dbl, _int, _int, _sz, _int])
_sig("fmrx_audio_meters_destroy", [_vp])
_sig("fmrx_audio_meters_reset", [_vp, _int])
_sig("fmrx_audio_meters_state_get", [_vp, _vp])
_sig("fmrx_audio_meters_process_dev", [_vp, _vp, _sz, _sz, _vp])
_sig("fmrx_audio_meters_collect", [_vp, _vp, _vp])
_sig("fmrx_audio_meters_process", [_vp, _vp, _sz, _sz, _vp, _vp])
_sig("fmrx_loudness_create", [C.POINTER(_vp), _int, _sz, _sz, _dbl])
_sig("fmrx_loudness_destroy", [_vp])
_sig("fmrx_loudness_reset", [_vp, _int])
_sig("fmrx_loudness_push", [_vp, _vp, _vp, _sz])
_sig("fmrx_loudness_read", [_vp, _int, _vp])


def _walk_rows(rows) -> np.ndarray:
    """One channel's rows for a host walk: float32 [audio_channels, n]; a single row may come flat."""
    x = _f32(rows)
    return x.reshape(1, -1) if x.ndim == 1 else x


def _levels_dict(out, dtype) -> dict:
    """One levels record as a dict, its arrays of 2 as tuples."""
    return {k: (tuple(float(v) for v in out[0][k]) if out[0][k].ndim else float(out[0][k])) for k in dtype.names}


def audioMetersDesign(audio_Fs) -> np.ndarray:
    """Host only: the K-weighting biquads for audio_Fs, float64 [2, 5]: (b0, b1, b2, a1, a2) of the shelf, then of the high-pass."""
    c = np.zeros(10)
    _check(lib.fmrx_audio_meters_design(float(audio_Fs), c))
    return c.reshape(2, 5)


def audioMetersBinLen(audio_Fs) -> int:
    """Host only: the samples of a 100 ms bin."""
    return lib.fmrx_audio_meters_bin_len(float(audio_Fs))


def audioMetersWalk(audio_Fs, rows, state=None):
    """Host only: the reference walk of one channel (fmrx_audio_meters_walk) on rows float32 [audio_channels, n]; state: the
    AUDIO_METER_STATE_DTYPE record the last call returned (None or zeros: a fresh channel) -> (record, bins [2, max_bins], state)."""
    x = _walk_rows(rows)
    st = np.zeros(1, AUDIO_METER_STATE_DTYPE) if state is None else np.array(state, dtype=AUDIO_METER_STATE_DTYPE).reshape(1).copy()
    rec = np.zeros(1, AUDIO_METER_DTYPE)
    nb = lib.fmrx_audio_meters_max_bins(float(audio_Fs), x.shape[1])
    bins = np.zeros((2, max(nb, 1)))
    _check(lib.fmrx_audio_meters_walk(float(audio_Fs), x.shape[0], x.ctypes.data, x.shape[1], x.shape[1], st.ctypes.data, rec.ctypes.data,
                                      bins.ctypes.data, bins.shape[1]))
    return rec[0], bins, st[0]


def audioMetersDerive(rec, audio_channels=2, full_scale=AUDIO_FULL_SCALE) -> dict:
    """Host only: the levels (fmrx_audio_levels, as a dict; the arrays of 2 as tuples) of one AUDIO_METER_DTYPE record."""
    r = np.array(rec, dtype=AUDIO_METER_DTYPE).reshape(1)
    out = np.zeros(1, AUDIO_LEVELS_DTYPE)
    _check(lib.fmrx_audio_meters_derive(r.ctypes.data, int(audio_channels), float(full_scale), out.ctypes.data))
    return _levels_dict(out, AUDIO_LEVELS_DTYPE)


class _AudioReader(_Handle):
    """What AudioMeters, TruePeak, AudioSpectrum, AudioFeatures and AudioResample share: a handle that only reads a bank's audio rows (csrc/meter_stage.hpp's Reader).  A
    subclass names its fmrx_<_prefix>_* functions and its module-level derive function, creates self._h, and says in _bank_extra
    what its constructor takes beyond n_channels, audio_channels, n_audio and device."""

    @classmethod
    def for_bank(cls, bank, *args, **kw):
        """The reader of a Channels bank, on the bank's device; further arguments as the class's _bank_extra takes them."""
        return cls(n_channels=bank.n_channels, audio_channels=bank.audio_channels, n_audio=bank.n_audio, device=bank.device,
                   **cls._bank_extra(bank, *args, **kw))

    def reset(self, channel=-1):
        self._call("reset", channel)

    def process_dev(self, d_audio, row_pitch=None, n=None, stream=None):
        """Device rows float32 [n_channels, audio_channels, row_pitch] of which the first n samples are walked (defaults: n_audio),
        asynchronous on `stream`; the rows are only read."""
        n = self.n_audio if n is None else int(n)
        self._call("process_dev", d_audio, n if row_pitch is None else int(row_pitch), n, stream)

    def process_bank(self, d_audio, stream=None):
        """process_dev on rows as the bank or any later stage wrote them: [n_channels, audio_channels, n_audio]."""
        self.process_dev(d_audio, self.n_audio, self.n_audio, stream)

    def _rows(self, audio) -> np.ndarray:    # the host call's rows
        return _f32(audio).reshape(self.n_channels, self.audio_channels, -1)

    def derive(self, rec, full_scale=AUDIO_FULL_SCALE) -> dict:
        return self._derive(rec, self.audio_channels, full_scale)


class AudioMeters(_AudioReader):
    """Per channel of a receiver bank and call: overs, peak, sums, K-weighted energy, the stereo cross sum and the 100 ms bins of
    the audio rows (fmrx_audio_meters_*).  The last stage of the chain, behind whatever wrote the rows on
    stream s: am = AudioMeters.for_bank(bank); am.process_bank(d_audio, stream=s); recs, bins = am.collect(); am.derive(recs[c]).
    It needs no Meters, so it also works behind the fused mono bank."""
    _prefix, _derive = "audio_meters", staticmethod(audioMetersDerive)
    _bank_extra = staticmethod(lambda bank: {"audio_Fs": bank.params.audio_Fs})

    def __init__(self, audio_Fs=48000.0, n_channels=1, audio_channels=2, n_audio=1920, device=0):
        self.audio_Fs, self.n_channels, self.audio_channels, self.n_audio = float(audio_Fs), int(n_channels), int(audio_channels), int(n_audio)
        self._h = _vp()
        _check(lib.fmrx_audio_meters_create(C.byref(self._h), self.audio_Fs, self.n_channels, self.audio_channels, self.n_audio, device))
        self.bin_len = lib.fmrx_audio_meters_bin_len(self.audio_Fs)
        self.max_bins = lib.fmrx_audio_meters_max_bins(self.audio_Fs, self.n_audio)

    def state(self) -> np.ndarray:
        """Waits for the last call; every channel's carried state, AUDIO_METER_STATE_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, AUDIO_METER_STATE_DTYPE)
        self._call("state_get", out.ctypes.data)
        return out

    def collect(self):
        """Waits for the last call; (AUDIO_METER_DTYPE [n_channels], bins float64 [n_channels, 2, max_bins])."""
        out, bins = np.zeros(self.n_channels, AUDIO_METER_DTYPE), np.zeros((self.n_channels, 2, self.max_bins))
        self._call("collect", out.ctypes.data, bins.ctypes.data)
        return out, bins

    def process(self, audio):
        """Host rows float32 [n_channels, audio_channels, n], n <= n_audio, synchronous -> what collect() returns."""
        x = self._rows(audio)
        out, bins = np.zeros(self.n_channels, AUDIO_METER_DTYPE), np.zeros((self.n_channels, 2, self.max_bins))
        self._call("process", x.ctypes.data, x.shape[2], x.shape[2], out.ctypes.data, bins.ctypes.data)
        return out, bins


class Loudness(_Handle):
    """Gated loudness by ITU-R BS.1770-4 over the audio meters' bins (fmrx_loudness_*), host only: loud = Loudness.for_meters(am);
    loud.push(*am.collect()); loud.read(c) -> momentary, short_term, integrated (LKFS), blocks, full."""
    _destroy = "fmrx_loudness_destroy"

    def __init__(self, n_channels, bin_len, max_blocks=36000, full_scale=AUDIO_FULL_SCALE):
        self.n_channels = int(n_channels)
        self._h = _vp()
        _check(lib.fmrx_loudness_create(C.byref(self._h), self.n_channels, int(bin_len), int(max_blocks), float(full_scale)))

    @classmethod
    def for_meters(cls, am, max_blocks=36000, full_scale=AUDIO_FULL_SCALE):
        return cls(am.n_channels, am.bin_len, max_blocks, full_scale)

    def reset(self, channel=-1):
        _check(lib.fmrx_loudness_reset(self._h, channel))

    def push(self, recs, bins):
        """What AudioMeters.collect() returned: records [n_channels] and bins [n_channels, 2, max_bins]."""
        r = np.ascontiguousarray(recs, dtype=AUDIO_METER_DTYPE).reshape(self.n_channels)
        b = np.ascontiguousarray(bins, dtype=np.float64).reshape(self.n_channels, 2, -1)
        _check(lib.fmrx_loudness_push(self._h, r.ctypes.data, b.ctypes.data, b.shape[2]))

    def read(self, channel=0) -> dict:
        out = np.zeros(1, LOUDNESS_LEVELS_DTYPE)
        _check(lib.fmrx_loudness_read(self._h, int(channel), out.ctypes.data))
        return dict(momentary=float(out[0]["momentary"]), short_term=float(out[0]["short_term"]), integrated=float(out[0]["integrated"]),
                    blocks=int(out[0]["blocks"]), full=bool(out[0]["full"]))


# --------------------------------------------------------------------------
# Loudness leveller and look-ahead peak limiter behind the audio meters
# --------------------------------------------------------------------------
class LevellerParams(C.Structure):
    """struct fmrx_leveller_params: target_lkfs / gate_lkfs in LKFS, max_boost_db / max_cut_db >= 0, attack / release per call in
    (0, 1], ceiling_dbfs < 0, full_scale the float value of 0 dBFS.  LevellerParams() holds the library's defaults; keyword
    arguments replace single fields.  max_boost_db = max_cut_db = 0 is a limiter alone."""
    _fields_ = [(k, C.c_double) for k in ("target_lkfs", "max_boost_db", "max_cut_db", "gate_lkfs", "attack", "release", "ceiling_dbfs",
                                          "full_scale")]

    def __init__(self, **kw):
        _params_init(self, lib.fmrx_leveller_defaults, kw)


LEVELLER_STATUS_DTYPE = np.dtype([("loud_ms", "<f8"), ("gain", "<f8"), ("gain0", "<f4"), ("gain1", "<f4"), ("gated", "<u4"),
                                  ("min_code", "<u4"), ("limited", "<u4"), ("reserved", "<u4"), ("calls", "<u8")])   # struct fmrx_leveller_status
LEVELLER_LEVELS_DTYPE = np.dtype([("loudness_lkfs", "<f8"), ("gain_db", "<f8"), ("reduction_db", "<f8")])          # struct fmrx_leveller_levels
LEVELLER_ONE = 1 << 24    # the gain code of "no reduction"
assert LEVELLER_STATUS_DTYPE.itemsize == 48 and LEVELLER_LEVELS_DTYPE.itemsize == 24 and C.sizeof(LevellerParams) == 64
_sig("fmrx_leveller_defaults", [C.POINTER(LevellerParams)])
_sig("fmrx_leveller_control", [C.POINTER(LevellerParams), _int, _vp, _vp])
_sig("fmrx_leveller_ceiling", [C.POINTER(LevellerParams), C.POINTER(C.c_float)])
_sig("fmrx_leveller_derive", [_vp, _vp])
_sig("fmrx_leveller_tile", [_int], _sz)
_sig("fmrx_leveller_walk", [_int, _int, C.c_float, C.c_float, C.c_float, _vp, _sz, _sz, _vp, _vp, _vp, _sz, C.POINTER(C.c_uint32),
                            C.POINTER(C.c_uint32)])
_sig("fmrx_leveller_create", [C.POINTER(_vp), C.POINTER(LevellerParams), _dbl, _int, _int, _sz, _int, _int])
_sig("fmrx_leveller_destroy", [_vp])
_sig("fmrx_leveller_reset", [_vp, _int])
_sig("fmrx_leveller_latency", [_vp], _sz)
_sig("fmrx_leveller_process_dev", [_vp, _vp, _vp, _vp, _vp, _int, _vp])
_sig("fmrx_leveller_process", [_vp, _vp, _vp, _vp, _vp, _int])
_sig("fmrx_leveller_status_get", [_vp, _vp])


def levellerControl(params, rec, state=None, audio_channels=2) -> np.ndarray:
    """Host only: one channel's control step (fmrx_leveller_control) on one AUDIO_METER_DTYPE record; state: the
    LEVELLER_STATUS_DTYPE record the last step returned (None or zeros: a fresh channel) -> the new one."""
    r = np.array(rec, dtype=AUDIO_METER_DTYPE).reshape(1)
    st = np.zeros(1, LEVELLER_STATUS_DTYPE) if state is None else np.array(state, dtype=LEVELLER_STATUS_DTYPE).reshape(1).copy()
    p = params if params is not None else LevellerParams()
    _check(lib.fmrx_leveller_control(C.byref(p), int(audio_channels), r.ctypes.data, st.ctypes.data))
    return st[0]


def levellerCeiling(params=None) -> np.float32:
    """Host only: the limiter's ceiling as the float32 the kernels compare with."""
    c = C.c_float()
    _check(lib.fmrx_leveller_ceiling(C.byref(params if params is not None else LevellerParams()), C.byref(c)))
    return np.float32(c.value)


def levellerTile(lookahead=64) -> int:
    """Host only: the samples of a row one workgroup of the apply kernel writes."""
    return lib.fmrx_leveller_tile(int(lookahead))


def levellerDerive(status) -> dict:
    """Host only: loudness_lkfs, gain_db and reduction_db of one LEVELLER_STATUS_DTYPE record."""
    st = np.array(status, dtype=LEVELLER_STATUS_DTYPE).reshape(1)
    out = np.zeros(1, LEVELLER_LEVELS_DTYPE)
    _check(lib.fmrx_leveller_derive(st.ctypes.data, out.ctypes.data))
    return {k: float(out[0][k]) for k in LEVELLER_LEVELS_DTYPE.names}


def levellerWalk(rows, gain0=1.0, gain1=1.0, lookahead=64, ceiling=None, state=None):
    """Host only: the serial reference of one channel's gain and limiter (fmrx_leveller_walk) on rows float32
    [audio_channels, n]; state: the (codes uint32 [2W-2], u float32 [audio_channels, W-1]) the last call returned (None: a fresh
    channel) -> (out [audio_channels, n], state, min_code, limited)."""
    x = _walk_rows(rows)
    ac, n, W = x.shape[0], x.shape[1], int(lookahead)
    if state is None:
        codes, u = np.full(max(2 * W - 2, 1), LEVELLER_ONE, np.uint32), np.zeros((ac, max(W - 1, 1)), np.float32)
    else:
        codes, u = np.array(state[0], dtype=np.uint32), np.array(state[1], dtype=np.float32).reshape(ac, -1)
    out = np.zeros((ac, n), np.float32)
    mn, cnt = C.c_uint32(), C.c_uint32()
    c = levellerCeiling() if ceiling is None else ceiling
    _check(lib.fmrx_leveller_walk(ac, W, float(c), float(gain0), float(gain1), x.ctypes.data, n, n, codes.ctypes.data, u.ctypes.data,
                                  out.ctypes.data, n, C.byref(mn), C.byref(cnt)))
    return out, (codes, u), mn.value, cnt.value


class Leveller(_MeterStage):
    """A gain towards a loudness target and a look-ahead peak limiter per channel of a receiver bank, decided from the audio
    meters' K-weighted sums of the same call (fmrx_leveller_*).  The last stage of the chain, and the one
    that packs the PCM: lv = Leveller.for_bank(bank, audio_meters); after audio_meters.process_bank(d_audio, stream=s):
    lv.process_bank(d_audio, d_out, d_pcm, stream=s); lv.status().  The output is delayed by lv.latency samples; d_out must not
    overlap d_audio."""

    _prefix, _status_dtype, _rec_dtype = "leveller", LEVELLER_STATUS_DTYPE, AUDIO_METER_DTYPE

    def __init__(self, audio_Fs=48000.0, n_channels=1, audio_channels=2, n_audio=1920, params: LevellerParams | None = None, lookahead=64,
                 device=0):
        self.audio_Fs, self.n_channels, self.audio_channels, self.n_audio = float(audio_Fs), int(n_channels), int(audio_channels), int(n_audio)
        self.params = params if params is not None else LevellerParams()
        self.lookahead = int(lookahead)
        self._meters = None
        self._h = _vp()
        _check(lib.fmrx_leveller_create(C.byref(self._h), C.byref(self.params), self.audio_Fs, self.n_channels, self.audio_channels,
                                        self.n_audio, self.lookahead, device))
        self.latency = lib.fmrx_leveller_latency(self._h)
        self.tile = lib.fmrx_leveller_tile(self.latency + 1)
        self.ceiling = levellerCeiling(self.params)

    @classmethod
    def for_bank(cls, bank, audio_meters, params: LevellerParams | None = None, lookahead=64):
        """The leveller of a Channels bank and of the AudioMeters made for it, on the bank's device."""
        lv = cls(bank.params.audio_Fs, bank.n_channels, bank.audio_channels, bank.n_audio, params, lookahead, bank.device)
        lv._meters = audio_meters
        return lv

    def derive(self, status) -> dict:
        return levellerDerive(status)


# --------------------------------------------------------------------------
# True-peak meter: the 4x oversampled peak (dBTP) of every audio row of a bank
# --------------------------------------------------------------------------
TRUE_PEAK_DTYPE = np.dtype([("n", "<u8"), ("over", "<u8", (2,)), ("true_peak", "<f8", (2,)), ("peak", "<f8", (2,))])    # struct fmrx_true_peak_record
TRUE_PEAK_LEVELS_DTYPE = np.dtype([("true_peak_dbtp", "<f8", (2,)), ("peak_dbfs", "<f8", (2,)), ("max_dbtp", "<f8"),
                                   ("over_fraction", "<f8")])                                                        # struct fmrx_true_peak_levels
assert TRUE_PEAK_DTYPE.itemsize == 56 and TRUE_PEAK_LEVELS_DTYPE.itemsize == 48
TRUE_PEAK_CARRY = 11                                                   # samples of a row carried from call to call
TRUE_PEAK_LIMIT = np.float32(AUDIO_FULL_SCALE * 10.0 ** (-1.0 / 20.0))   # -1 dBTP
_sig("fmrx_true_peak_taps", [_f32p])
_sig("fmrx_true_peak_latency", [], _sz)
_sig("fmrx_true_peak_tile", [], _sz)
_sig("fmrx_true_peak_walk", [_int, _vp, _sz, _sz, _flt, _vp, _vp])
_sig("fmrx_true_peak_derive", [_vp, _int, _dbl, _vp])
_sig("fmrx_true_peak_create", [C.POINTER(_vp), _int, _int, _sz, _flt, _int])
_sig("fmrx_true_peak_destroy", [_vp])
_sig("fmrx_true_peak_reset", [_vp, _int])
_sig("fmrx_true_peak_state_get", [_vp, _vp])
_sig("fmrx_true_peak_process_dev", [_vp, _vp, _sz, _sz, _vp])
_sig("fmrx_true_peak_collect", [_vp, _vp])
_sig("fmrx_true_peak_process", [_vp, _vp, _sz, _sz, _vp])


def truePeakTaps() -> np.ndarray:
    """Host only: the interpolator's table, float32 [3, 12]: phases 1, 2, 3 (phase 0 is the sample itself)."""
    h = np.zeros(36, np.float32)
    _check(lib.fmrx_true_peak_taps(h))
    return h.reshape(3, 12)


def truePeakWalk(rows, state=None, limit=TRUE_PEAK_LIMIT):
    """Host only: the reference walk of one channel (fmrx_true_peak_walk) on rows float32 [audio_channels, n]; state: float32
    [2, 11], what the last call returned (None or zeros: a fresh channel) -> (record, state)."""
    x = _walk_rows(rows)
    st = np.zeros((2, TRUE_PEAK_CARRY), np.float32) if state is None else np.array(state, dtype=np.float32).reshape(2, TRUE_PEAK_CARRY).copy()
    rec = np.zeros(1, TRUE_PEAK_DTYPE)
    _check(lib.fmrx_true_peak_walk(x.shape[0], x.ctypes.data, x.shape[1], x.shape[1], float(limit), st.ctypes.data, rec.ctypes.data))
    return rec[0], st


def truePeakDerive(rec, audio_channels=2, full_scale=AUDIO_FULL_SCALE) -> dict:
    """Host only: the levels (fmrx_true_peak_levels, as a dict; the arrays of 2 as tuples) of one TRUE_PEAK_DTYPE record."""
    r = np.array(rec, dtype=TRUE_PEAK_DTYPE).reshape(1)
    out = np.zeros(1, TRUE_PEAK_LEVELS_DTYPE)
    _check(lib.fmrx_true_peak_derive(r.ctypes.data, int(audio_channels), float(full_scale), out.ctypes.data))
    return _levels_dict(out, TRUE_PEAK_LEVELS_DTYPE)


class TruePeak(_AudioReader):
    """Per channel of a receiver bank and call: the peak of the 4x oversampled waveform, the sample peak and the groups beyond
    `limit` of the audio rows (fmrx_true_peak_*).  Behind the last audio stage on stream s: tp =
    TruePeak.for_bank(bank); tp.process_bank(d_out, stream=s); recs = tp.collect(); tp.derive(recs[c]).  The reading lags the
    audio by tp.latency samples."""
    _prefix, _derive = "true_peak", staticmethod(truePeakDerive)
    _bank_extra = staticmethod(lambda bank, limit=TRUE_PEAK_LIMIT: {"limit": limit})

    def __init__(self, n_channels=1, audio_channels=2, n_audio=1920, limit=TRUE_PEAK_LIMIT, device=0):
        self.n_channels, self.audio_channels, self.n_audio, self.limit = int(n_channels), int(audio_channels), int(n_audio), np.float32(limit)
        self._h = _vp()
        _check(lib.fmrx_true_peak_create(C.byref(self._h), self.n_channels, self.audio_channels, self.n_audio, float(self.limit), device))
        self.latency = lib.fmrx_true_peak_latency()
        self.tile = lib.fmrx_true_peak_tile()

    def state(self) -> np.ndarray:
        """Waits for the last call; every channel's carried samples, float32 [n_channels, 2, 11]."""
        out = np.zeros((self.n_channels, 2, TRUE_PEAK_CARRY), np.float32)
        self._call("state_get", out.ctypes.data)
        return out

    def collect(self) -> np.ndarray:
        """Waits for the last call; TRUE_PEAK_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, TRUE_PEAK_DTYPE)
        self._call("collect", out.ctypes.data)
        return out

    def process(self, audio) -> np.ndarray:
        """Host rows float32 [n_channels, audio_channels, n], n <= n_audio, synchronous -> what collect() returns."""
        x = self._rows(audio)
        out = np.zeros(self.n_channels, TRUE_PEAK_DTYPE)
        self._call("process", x.ctypes.data, x.shape[2], x.shape[2], out.ctypes.data)
        return out


# --------------------------------------------------------------------------
# Audio spectrum meter: the band powers of every audio row of a bank
# --------------------------------------------------------------------------
AUDIO_SPECTRUM_DTYPE = np.dtype([("n", "<u8"), ("frames", "<u8"), ("band", "<f8", (2, 32))])                      # struct fmrx_audio_spectrum_record
AUDIO_SPECTRUM_STATE_DTYPE = np.dtype([("fill", "<u4"), ("carry", "<f4", (2, 255))])                              # struct fmrx_audio_spectrum_state
AUDIO_SPECTRUM_LEVELS_DTYPE = np.dtype([("band_dbfs", "<f8", (2, 32)), ("total_dbfs", "<f8", (2,)), ("centroid_hz", "<f8", (2,))])   # struct fmrx_audio_spectrum_levels
assert AUDIO_SPECTRUM_DTYPE.itemsize == 528 and AUDIO_SPECTRUM_STATE_DTYPE.itemsize == 2044 and AUDIO_SPECTRUM_LEVELS_DTYPE.itemsize == 544
_sig("fmrx_audio_spectrum_tables", [_f32p, _f32p])
_sig("fmrx_audio_spectrum_frame", [], _sz)
_sig("fmrx_audio_spectrum_bins", [], _sz)
_sig("fmrx_audio_spectrum_tile", [], _sz)
_sig("fmrx_audio_spectrum_max_bands", [], _sz)
_sig("fmrx_audio_spectrum_default_edges", [_vp, C.POINTER(_int)])
_sig("fmrx_audio_spectrum_walk", [_int, _vp, _sz, _sz, _vp, _int, _vp, _vp])
_sig("fmrx_audio_spectrum_derive", [_vp, _int, _vp, _int, _dbl, _dbl, _vp])
_sig("fmrx_audio_spectrum_create", [C.POINTER(_vp), _int, _int, _sz, _vp, _int, _int])
_sig("fmrx_audio_spectrum_destroy", [_vp])
_sig("fmrx_audio_spectrum_reset", [_vp, _int])
_sig("fmrx_audio_spectrum_state_get", [_vp, _vp])
_sig("fmrx_audio_spectrum_process_dev", [_vp, _vp, _sz, _sz, _vp])
_sig("fmrx_audio_spectrum_collect", [_vp, _vp])
_sig("fmrx_audio_spectrum_process", [_vp, _vp, _sz, _sz, _vp])


def audioSpectrumTables():
    """Host only: (w float32 [256], the periodic Hann window; C float32 [256], cos(2 pi m / 256)), the tables that define the meter."""
    w, c = np.zeros(256, np.float32), np.zeros(256, np.float32)
    _check(lib.fmrx_audio_spectrum_tables(w, c))
    return w, c


def audioSpectrumDefaultEdges() -> np.ndarray:
    """Host only: the default band edges, int32 [24]: 23 bands."""
    e, nb = np.zeros(33, np.int32), _int()
    _check(lib.fmrx_audio_spectrum_default_edges(e.ctypes.data, C.byref(nb)))
    return e[:nb.value + 1].copy()


def _spectrum_edges(edges):
    """-> (int32 array or None, its pointer or None, n_bands) as the library's edges / n_bands arguments take them"""
    if edges is None:
        return None, None, 0
    e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
    return e, e.ctypes.data, len(e) - 1


def audioSpectrumWalk(rows, state=None, edges=None):
    """Host only: the reference walk of one channel (fmrx_audio_spectrum_walk) on rows float32 [audio_channels, n]; state: the
    AUDIO_SPECTRUM_STATE_DTYPE record the last call returned (None or zeros: a fresh channel); edges: None for the default bands
    -> (record, state)."""
    x = _walk_rows(rows)
    st = np.zeros(1, AUDIO_SPECTRUM_STATE_DTYPE) if state is None else np.array(state, dtype=AUDIO_SPECTRUM_STATE_DTYPE).reshape(1).copy()
    rec = np.zeros(1, AUDIO_SPECTRUM_DTYPE)
    e, ep, nb = _spectrum_edges(edges)
    _check(lib.fmrx_audio_spectrum_walk(x.shape[0], x.ctypes.data, x.shape[1], x.shape[1], ep, nb, st.ctypes.data, rec.ctypes.data))
    return rec[0], st[0]


def audioSpectrumDerive(rec, audio_channels=2, edges=None, audio_Fs=48000.0, full_scale=AUDIO_FULL_SCALE) -> dict:
    """Host only: the levels (fmrx_audio_spectrum_levels) of one AUDIO_SPECTRUM_DTYPE record, as a dict of float64 arrays:
    band_dbfs [2, 32], total_dbfs [2], centroid_hz [2]."""
    r = np.array(rec, dtype=AUDIO_SPECTRUM_DTYPE).reshape(1)
    out = np.zeros(1, AUDIO_SPECTRUM_LEVELS_DTYPE)
    e, ep, nb = _spectrum_edges(edges)
    _check(lib.fmrx_audio_spectrum_derive(r.ctypes.data, int(audio_channels), ep, nb, float(audio_Fs), float(full_scale), out.ctypes.data))
    return {k: out[0][k].copy() for k in AUDIO_SPECTRUM_LEVELS_DTYPE.names}


class AudioSpectrum(_AudioReader):
    """Per channel of a receiver bank and call: the power in up to 32 frequency bands of each audio row, summed over the
    256-sample frames the call completed (fmrx_audio_spectrum_*).  Behind the last audio stage on stream s:
    sp = AudioSpectrum.for_bank(bank); sp.process_bank(d_out, stream=s); recs = sp.collect(); sp.derive(recs[c]).  edges: None
    for the 23 default bands, or B + 1 bin numbers ascending within 1 .. 128."""
    _prefix = "audio_spectrum"
    _bank_extra = staticmethod(lambda bank, edges=None: {"edges": edges, "audio_Fs": bank.params.audio_Fs})

    def __init__(self, n_channels=1, audio_channels=2, n_audio=1920, edges=None, audio_Fs=48000.0, device=0):
        self.n_channels, self.audio_channels, self.n_audio, self.audio_Fs = int(n_channels), int(audio_channels), int(n_audio), float(audio_Fs)
        e, ep, nb = _spectrum_edges(edges)
        self._h = _vp()
        _check(lib.fmrx_audio_spectrum_create(C.byref(self._h), self.n_channels, self.audio_channels, self.n_audio, ep, nb, device))
        self.edges = audioSpectrumDefaultEdges() if e is None else e.copy()
        self.n_bands = len(self.edges) - 1
        self.frame = lib.fmrx_audio_spectrum_frame()
        self.tile = lib.fmrx_audio_spectrum_tile()

    def band_hz(self) -> np.ndarray:
        """The centre frequency of every band, float64 [n_bands]: what the centroid weighs the bands with."""
        e = self.edges.astype(np.float64)
        return (e[:-1] + e[1:] - 1.0) / 2.0 * (self.audio_Fs / self.frame)

    def derive(self, rec, full_scale=AUDIO_FULL_SCALE) -> dict:
        return audioSpectrumDerive(rec, self.audio_channels, self.edges, self.audio_Fs, full_scale)

    def state(self) -> np.ndarray:
        """Waits for the last call; every channel's carried state, AUDIO_SPECTRUM_STATE_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, AUDIO_SPECTRUM_STATE_DTYPE)
        self._call("state_get", out.ctypes.data)
        return out

    def collect(self) -> np.ndarray:
        """Waits for the last call; AUDIO_SPECTRUM_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, AUDIO_SPECTRUM_DTYPE)
        self._call("collect", out.ctypes.data)
        return out

    def process(self, audio) -> np.ndarray:
        """Host rows float32 [n_channels, audio_channels, n], n <= n_audio, synchronous -> what collect() returns."""
        x = self._rows(audio)
        out = np.zeros(self.n_channels, AUDIO_SPECTRUM_DTYPE)
        self._call("process", x.ctypes.data, x.shape[2], x.shape[2], out.ctypes.data)
        return out


# --------------------------------------------------------------------------
# Audio feature frames: a mel-band spectrogram of every channel of a bank
# --------------------------------------------------------------------------
class AudioFeaturesParams(C.Structure):
    """struct fmrx_audio_features_params (include/fmrx.h): the geometry of the feature frames."""
    _fields_ = [("win", C.c_uint32), ("hop", C.c_uint32), ("n_bins", C.c_uint32), ("n_mels", C.c_uint32), ("f_lo", _dbl), ("f_hi", _dbl),
                ("audio_Fs", _dbl)]


AUDIO_FEATURES_STATE_DTYPE = np.dtype([("fill", "<u4"), ("carry", "<f4", (1279,))])                                # struct fmrx_audio_features_state
assert C.sizeof(AudioFeaturesParams) == 40 and AUDIO_FEATURES_STATE_DTYPE.itemsize == 5120
_afp = C.POINTER(AudioFeaturesParams)
_sig("fmrx_audio_features_preset", [_dbl, _afp])
_sig("fmrx_audio_features_tables", [_afp, _vp, _vp, _vp, _vp, _vp])
_sig("fmrx_audio_features_max_frames", [_afp, _sz], _sz)
_sig("fmrx_audio_features_walk", [_afp, _int, _vp, _sz, _sz, _vp, _vp, _vp])
_sig("fmrx_audio_features_create", [C.POINTER(_vp), _afp, _int, _int, _sz, _int])
_sig("fmrx_audio_features_destroy", [_vp])
_sig("fmrx_audio_features_reset", [_vp, _int])
_sig("fmrx_audio_features_state_get", [_vp, _vp])
_sig("fmrx_audio_features_process_dev", [_vp, _vp, _sz, _sz, _vp])
_sig("fmrx_audio_features_result_dev", [_vp, C.POINTER(_vp), C.POINTER(_vp)])
_sig("fmrx_audio_features_collect", [_vp, _vp, _vp])
_sig("fmrx_audio_features_process", [_vp, _vp, _sz, _sz, _vp, _vp])


def _features_params(params) -> AudioFeaturesParams:
    """An AudioFeaturesParams from one, from a dict of its fields, or from (win, hop, n_bins, n_mels, f_lo, f_hi, audio_Fs)."""
    if isinstance(params, AudioFeaturesParams):
        return params
    if isinstance(params, dict):
        return AudioFeaturesParams(**params)
    return AudioFeaturesParams(*params)


def audioFeaturesPreset(audio_Fs=48000.0) -> AudioFeaturesParams:
    """Host only: the speech-model geometry for an audio rate of 48 000 or 44 100 Hz (fmrx_audio_features_preset)."""
    p = AudioFeaturesParams()
    _check(lib.fmrx_audio_features_preset(float(audio_Fs), C.byref(p)))
    return p


def audioFeaturesTables(params) -> dict:
    """Host only: the float32 tables that define the stage for a geometry (fmrx_audio_features_tables): window [win], cosine [win],
    mel_lo and mel_hi int32 [n_mels], mel_w [n_mels, n_bins]."""
    p = _features_params(params)
    shape = (max(int(p.n_mels), 1), max(int(p.n_bins), 1))
    t = dict(window=np.zeros(max(int(p.win), 1), np.float32), cosine=np.zeros(max(int(p.win), 1), np.float32), mel_lo=np.zeros(shape[0], np.int32),
             mel_hi=np.zeros(shape[0], np.int32), mel_w=np.zeros(shape, np.float32))
    _check(lib.fmrx_audio_features_tables(C.byref(p), *(t[k].ctypes.data for k in ("window", "cosine", "mel_lo", "mel_hi", "mel_w"))))
    return t


def audioFeaturesMaxFrames(params, n_audio) -> int:
    """Host only: the most frames a call of n_audio samples completes, (n_audio - 1) // hop + 1; 0 for a refused geometry."""
    return int(lib.fmrx_audio_features_max_frames(C.byref(_features_params(params)), int(n_audio)))


def audioFeaturesWalk(rows, params, state=None):
    """Host only: the reference walk of one channel (fmrx_audio_features_walk) on rows float32 [audio_channels, n]; state: the
    AUDIO_FEATURES_STATE_DTYPE record the last call returned (None or zeros: a fresh channel) -> (feat float32 [F_max(n), n_mels],
    frames, state)."""
    p = _features_params(params)
    x = _walk_rows(rows)
    st = np.zeros(1, AUDIO_FEATURES_STATE_DTYPE) if state is None else np.array(state, dtype=AUDIO_FEATURES_STATE_DTYPE).reshape(1).copy()
    feat = np.zeros((max(audioFeaturesMaxFrames(p, x.shape[1]), 1), max(int(p.n_mels), 1)), np.float32)
    frames = np.zeros(1, np.uint32)
    _check(lib.fmrx_audio_features_walk(C.byref(p), x.shape[0], x.ctypes.data, x.shape[1], x.shape[1], st.ctypes.data, feat.ctypes.data, frames.ctypes.data))
    return feat, int(frames[0]), st[0]


class AudioFeatures(_AudioReader):
    """Per channel of a receiver bank: a mel-band spectrogram of the channel's mono mix, n_mels linear powers per frame of win
    samples every hop samples, across calls (fmrx_audio_features_*).  Behind the last audio stage on stream
    s: af = AudioFeatures.for_bank(bank); af.process_bank(d_out, stream=s); ptr, frames_ptr, shape = af.result_dev() for a
    consumer on the device, or feat, frames = af.collect().  params: None for the preset of the audio rate."""
    _prefix = "audio_features"
    _bank_extra = staticmethod(lambda bank, params=None: {"params": audioFeaturesPreset(bank.params.audio_Fs) if params is None else params})

    def __init__(self, n_channels=1, audio_channels=2, n_audio=1920, params=None, device=0):
        self.n_channels, self.audio_channels, self.n_audio = int(n_channels), int(audio_channels), int(n_audio)
        self.params = audioFeaturesPreset(48000.0) if params is None else _features_params(params)
        self._h = _vp()
        _check(lib.fmrx_audio_features_create(C.byref(self._h), C.byref(self.params), self.n_channels, self.audio_channels, self.n_audio, device))
        self.n_mels = int(self.params.n_mels)
        self.max_frames = audioFeaturesMaxFrames(self.params, self.n_audio)

    def _results(self):
        return np.zeros((self.n_channels, self.max_frames, self.n_mels), np.float32), np.zeros(self.n_channels, np.uint32)

    def state(self) -> np.ndarray:
        """Waits for the last call; every channel's carried state, AUDIO_FEATURES_STATE_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, AUDIO_FEATURES_STATE_DTYPE)
        self._call("state_get", out.ctypes.data)
        return out

    def result_dev(self):
        """(feat_ptr, frames_ptr, (n_channels, F_max, n_mels)): the last call's float32 features and uint32 frame counts on the
        device, ordered behind the call on its stream and valid until the handle's next call."""
        feat, frames = _vp(), _vp()
        self._call("result_dev", C.byref(feat), C.byref(frames))
        return feat.value, frames.value, (self.n_channels, self.max_frames, self.n_mels)

    def collect(self):
        """Waits for the last call; (feat float32 [n_channels, F_max, n_mels], frames uint32 [n_channels])."""
        feat, frames = self._results()
        self._call("collect", feat.ctypes.data, frames.ctypes.data)
        return feat, frames

    def process(self, audio):
        """Host rows float32 [n_channels, audio_channels, n], n <= n_audio, synchronous -> what collect() returns."""
        x = self._rows(audio)
        feat, frames = self._results()
        self._call("process", x.ctypes.data, x.shape[2], x.shape[2], feat.ctypes.data, frames.ctypes.data)
        return feat, frames


# --------------------------------------------------------------------------
# Audio rate converter: a bank's audio at 16 kHz mono or any rate up / down
# --------------------------------------------------------------------------
class AudioResampleParams(C.Structure):
    """struct fmrx_audio_resample_params (include/fmrx.h): the geometry of the rate converter."""
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32), ("mix", C.c_uint32), ("cutoff", _dbl), ("beta", _dbl)]

    @classmethod
    def preset(cls, audio_Fs, out_Fs, mix=True):
        """Host only: the geometry that takes audio_Fs to out_Fs, two integer rates within 8 000 .. 48 000 (fmrx_audio_resample_preset)."""
        p = cls()
        _check(lib.fmrx_audio_resample_preset(float(audio_Fs), float(out_Fs), int(bool(mix)), C.byref(p)))
        return p


AUDIO_RESAMPLE_STATE_DTYPE = np.dtype([("pos", "<u4"), ("reserved", "<u4"), ("carry", "<f4", (2, 255))])          # struct fmrx_audio_resample_state
assert C.sizeof(AudioResampleParams) == 32 and AUDIO_RESAMPLE_STATE_DTYPE.itemsize == 2048
_arp = C.POINTER(AudioResampleParams)
_sig("fmrx_audio_resample_preset", [_dbl, _dbl, _int, _arp])
_sig("fmrx_audio_resample_taps", [_arp, _vp])
_sig("fmrx_audio_resample_max_out", [_arp, _sz], _sz)
_sig("fmrx_audio_resample_latency", [_arp], _dbl)
_sig("fmrx_audio_resample_walk", [_arp, _int, _vp, _sz, _sz, _vp, _vp, _vp])
_sig("fmrx_audio_resample_create", [C.POINTER(_vp), _arp, _int, _int, _sz, _int, _int, _int])
_sig("fmrx_audio_resample_destroy", [_vp])
_sig("fmrx_audio_resample_reset", [_vp, _int])
_sig("fmrx_audio_resample_state_get", [_vp, _vp])
_sig("fmrx_audio_resample_process_dev", [_vp, _vp, _sz, _sz, _int, _vp])
_sig("fmrx_audio_resample_result_dev", [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)])
_sig("fmrx_audio_resample_collect", [_vp, _vp, _vp, _vp])
_sig("fmrx_audio_resample_process", [_vp, _vp, _sz, _sz, _int, _vp, _vp, _vp])


def _resample_params(params) -> AudioResampleParams:
    """An AudioResampleParams from one, from a dict of its fields, or from (up, down, taps, mix, cutoff, beta)."""
    if isinstance(params, AudioResampleParams):
        return params
    if isinstance(params, dict):
        return AudioResampleParams(**params)
    return AudioResampleParams(*params)


def audioResamplePreset(audio_Fs=48000.0, out_Fs=16000.0, mix=True) -> AudioResampleParams:
    """Host only: AudioResampleParams.preset."""
    return AudioResampleParams.preset(audio_Fs, out_Fs, mix)


def audioResampleTaps(params) -> np.ndarray:
    """Host only: the float32 taps that define the converter for a geometry, [up, taps] phase-major (fmrx_audio_resample_taps)."""
    p = _resample_params(params)
    h = np.zeros((max(int(p.up), 1), max(int(p.taps), 1)), np.float32)
    _check(lib.fmrx_audio_resample_taps(C.byref(p), h.ctypes.data))
    return h


def audioResampleMaxOut(params, n_audio) -> int:
    """Host only: the most outputs a call of n_audio samples completes, ceil(n_audio up / down); 0 for a refused geometry."""
    return int(lib.fmrx_audio_resample_max_out(C.byref(_resample_params(params)), int(n_audio)))


def audioResampleLatency(params) -> float:
    """Host only: the group delay (up taps - 1) / (2 up) in input samples; NaN for a refused geometry."""
    return float(lib.fmrx_audio_resample_latency(C.byref(_resample_params(params))))


def audioResampleWalk(rows, params, state=None):
    """Host only: the reference walk of one channel (fmrx_audio_resample_walk) on rows float32 [audio_channels, n]; state: the
    AUDIO_RESAMPLE_STATE_DTYPE record the last call returned (None or zeros: a fresh channel) -> (out float32 [R, M_max(n)], count,
    state)."""
    p = _resample_params(params)
    x = _walk_rows(rows)
    st = np.zeros(1, AUDIO_RESAMPLE_STATE_DTYPE) if state is None else np.array(state, dtype=AUDIO_RESAMPLE_STATE_DTYPE).reshape(1).copy()
    out = np.zeros((1 if p.mix else x.shape[0], max(audioResampleMaxOut(p, x.shape[1]), 1)), np.float32)
    count = np.zeros(1, np.uint32)
    _check(lib.fmrx_audio_resample_walk(C.byref(p), x.shape[0], x.ctypes.data, x.shape[1], x.shape[1], st.ctypes.data, out.ctypes.data, count.ctypes.data))
    return out, int(count[0]), st[0]


class AudioResample(_AudioReader):
    """Per channel of a receiver bank: the channel's mono mix (params.mix) or each of its rows at the rate up / down, history and
    phase carried across calls (fmrx_audio_resample_*).  Behind the last audio stage on stream s:
    ar = AudioResample.for_bank(bank, AudioResampleParams.preset(48000, 16000)); ar.process_bank(d_out, stream=s);
    f32_ptr, pcm_ptr, counts_ptr, shape = ar.result_dev() for a consumer on the device, or out = ar.collect().  params: None for
    the preset that takes the audio rate to 16 kHz mono."""
    _prefix = "audio_resample"
    _bank_extra = staticmethod(lambda bank, params=None, want_f32=True, want_pcm=False: {
        "params": AudioResampleParams.preset(bank.params.audio_Fs, 16000.0) if params is None else params, "want_f32": want_f32, "want_pcm": want_pcm})

    def __init__(self, n_channels=1, audio_channels=2, n_audio=1920, params=None, want_f32=True, want_pcm=False, device=0):
        self.n_channels, self.audio_channels, self.n_audio = int(n_channels), int(audio_channels), int(n_audio)
        self.params = AudioResampleParams.preset(48000.0, 16000.0) if params is None else _resample_params(params)
        self.want_f32, self.want_pcm = bool(want_f32), bool(want_pcm)
        self._h = _vp()
        _check(lib.fmrx_audio_resample_create(C.byref(self._h), C.byref(self.params), self.n_channels, self.audio_channels, self.n_audio,
                                              int(self.want_f32), int(self.want_pcm), device))
        self.rows = 1 if self.params.mix else self.audio_channels
        self.max_out = audioResampleMaxOut(self.params, self.n_audio)
        self.latency = audioResampleLatency(self.params)

    @property
    def shape(self):
        return (self.n_channels, self.rows, self.max_out)

    def _results(self):
        return dict(audio=np.zeros(self.shape, np.float32) if self.want_f32 else None, pcm16=np.zeros(self.shape, np.int16) if self.want_pcm else None,
                    counts=np.zeros(self.n_channels, np.uint32))

    @staticmethod
    def _ptrs(out):
        return tuple(None if out[k] is None else out[k].ctypes.data for k in ("audio", "pcm16", "counts"))

    def process_dev(self, d_audio, row_pitch=None, n=None, stream=None, wrap=True):
        """Device rows float32 [n_channels, audio_channels, row_pitch] of which the first n samples are walked (defaults: n_audio),
        asynchronous on `stream`; the rows are only read.  wrap: the PCM pack's policy."""
        n = self.n_audio if n is None else int(n)
        self._call("process_dev", d_audio, n if row_pitch is None else int(row_pitch), n, PCM_WRAP if wrap else PCM_SATURATE, stream)

    def process_bank(self, d_audio, stream=None, wrap=True):
        """process_dev on rows as the bank or any later stage wrote them: [n_channels, audio_channels, n_audio]."""
        self.process_dev(d_audio, self.n_audio, self.n_audio, stream, wrap)

    def state(self) -> np.ndarray:
        """Waits for the last call; every channel's carried state, AUDIO_RESAMPLE_STATE_DTYPE [n_channels]."""
        out = np.zeros(self.n_channels, AUDIO_RESAMPLE_STATE_DTYPE)
        self._call("state_get", out.ctypes.data)
        return out

    def result_dev(self):
        """(f32_ptr, pcm_ptr, counts_ptr, (n_channels, R, M_max)): the last call's float32 and int16 rows (None for the one the handle
        does not keep) and uint32 counts on the device, ordered behind the call on its stream and valid until the handle's next call."""
        f32, pcm, counts = _vp(), _vp(), _vp()
        self._call("result_dev", C.byref(f32), C.byref(pcm), C.byref(counts))
        return f32.value, pcm.value, counts.value, self.shape

    def collect(self) -> dict:
        """Waits for the last call; dict(audio float32 [n_channels, R, M_max] or None, pcm16 int16 of that shape or None, counts uint32
        [n_channels])."""
        out = self._results()
        self._call("collect", *self._ptrs(out))
        return out

    def process(self, audio, wrap=True) -> dict:
        """Host rows float32 [n_channels, audio_channels, n], n <= n_audio, synchronous -> what collect() returns."""
        x = self._rows(audio)
        out = self._results()
        self._call("process", x.ctypes.data, x.shape[2], x.shape[2], PCM_WRAP if wrap else PCM_SATURATE, *self._ptrs(out))
        return out


class FrontEndPlan(_Handle):
    """Reusable device-side tap tables for the fused front-end kernel (fmrx_fe_plan)."""
    _destroy = "fmrx_fe_plan_destroy"

    def __init__(self, h, decim):
        h = _f32(h)
        self.taps, self.decim = len(h), int(decim)
        self._h = _vp()
        _check(lib.fmrx_fe_plan_create(C.byref(self._h), h, len(h), decim))

    @property
    def specialised(self) -> bool:
        return bool(lib.fmrx_fe_plan_is_specialised(self._h))

    @property
    def history_bytes(self) -> int:
        return lib.fmrx_fe_plan_history_bytes(self._h)

    def run_dev(self, d_iq_ptr, n_samples, d_hist_ptr, d_if_ptr, force_generic=False, stream=None):
        _check(lib.fmrx_fe_run_dev(self._h, d_iq_ptr, n_samples, d_hist_ptr, d_if_ptr, int(force_generic), stream))
