"""RDS banks without a GPU: the Python mirror and the C ABI exist, argument checks come before any device call (FMRX_EINVAL),
a bank without a device is refused (FMRX_ENODEV, no CPU fallback), and the receiver-bank fixture of test_gpu_rds_bank.py is
meaningful: the oracle's receiver followed by the oracle's RDS chain recovers the transmitted bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def test_rds_bank_api_exists(fmrx):
    assert hasattr(fmrx, "RdsBank") and hasattr(fmrx.Channels, "demod_layout")
    for name in ("process", "process_dev", "collect", "reset", "read_tap", "close"):
        assert callable(getattr(fmrx.RdsBank, name)), name
    lib = C.CDLL(fmrx.LIB_PATH)
    for sym in ("fmrx_rds_bank_create", "fmrx_rds_bank_destroy", "fmrx_rds_bank_reset", "fmrx_rds_bank_n_out", "fmrx_rds_bank_max_bits",
                "fmrx_rds_bank_process_dev", "fmrx_rds_bank_collect", "fmrx_rds_bank_process", "fmrx_rds_bank_read_tap",
                "fmrx_channels_demod_layout"):
        assert hasattr(lib, sym), sym


def test_rds_bank_argument_checks_before_the_device(fmrx):
    def einval(fn, *a, **k):
        with pytest.raises(fmrx.FmrxError) as e:
            fn(*a, **k)
        assert e.value.code == fmrx.EINVAL, str(e.value)

    einval(fmrx.RdsBank, 0, 4, block=9601)                  # block*upsamp not a multiple of decim
    einval(fmrx.RdsBank, 2, 4, block=9600 + 960)            # mode 2: 817/1920
    einval(fmrx.RdsBank, 0, 0)                              # no channels
    einval(fmrx.RdsBank, 1, 4)                              # the model defines no RDS rates for mode 1
    einval(fmrx.RdsBank, n_channels=4, block=100, params=fmrx.RdsParams(240000, 151, 1, 1, 26, 101))   # shorter than a history
    einval(fmrx.RdsBank, n_channels=4, params=fmrx.RdsParams(240000, 2, 247, 960, 26, 101))           # bad parameters
    L = fmrx.lib
    sz = C.c_size_t(0)
    ptr = C.c_void_p()
    for rc in (L.fmrx_rds_bank_reset(None, 0), L.fmrx_rds_bank_process_dev(None, None, 9600, None),
               L.fmrx_rds_bank_collect(None, None, None, None, None, None), L.fmrx_rds_bank_read_tap(None, 0, 0, None, C.byref(sz)),
               L.fmrx_channels_demod_layout(None, C.byref(ptr), C.byref(sz), C.byref(sz))):
        assert rc == fmrx.EINVAL
    assert L.fmrx_rds_bank_n_out(None) == 0 and L.fmrx_rds_bank_max_bits(None) == 0
    assert L.fmrx_rds_bank_destroy(None) == fmrx.OK


def test_rds_bank_without_a_device(fmrx):
    if fmrx.device_count() > 0:                             # (on a GPU machine: the bank is made, with its sizes)
        bank = fmrx.RdsBank(0, 4, 9600)
        assert (bank.n_out, bank.max_bits) == (2470, 2470 // 26 + 4)
        bank.close()
        return
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.RdsBank(0, 4, 9600)
    assert e.value.code == fmrx.ENODEV


def test_receiver_bank_rds_fixture_is_meaningful(oracle):
    """The I/Q of test_receiver_bank_to_rds_bank_on_the_device through the oracle's receiver (which the exact bank equals bit for
    bit) and the oracle's RDS chain: within a block the recovered bits ARE the transmitted ones (>= 97 %, as
    test_rds_chain_against_the_reference_model checks for rds.npz), and the frame synchroniser finds offset words."""
    import rds_oracle as R
    from _rds_util import rds_iq_u8
    nb = 4
    for c in range(3):
        iq, tx = rds_iq_u8(nb, seed=5 + c, chip_offset=600.0 + 97 * c)
        pl, chain = oracle.pipeline(0, 2), R.RdsChain()
        synced = 0
        for b in range(nb):
            out = chain.process(pl.process(iq[b * 192000:(b + 1) * 192000])["demod"])
            got = out["diff_bits"].astype(np.uint8)[1:]
            assert len(got) >= 40
            assert max(np.mean(got == tx[s:s + len(got)]) for s in range(len(tx) - len(got))) >= 0.97, (c, b)
            synced += out["offset_type"] != " "
        assert synced >= 2, c
