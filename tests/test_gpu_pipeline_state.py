"""fmrx_pipeline_get_state / set_state: the project's checkpoint and resume, beyond the one point test_state_round_trip pins.

A stream is five unequal blocks b0..b4 of 2 000 - 3 000 IF samples (modes 2 / 3: whole resampler periods).  Handle A processes
b0, b1, serialises its state and goes on with b2, b3, b4.  Handles B take that state and process b2, b3, b4 as well: a fresh one,
one that has processed one block of ANOTHER stream and one that has processed two -- which leaves the handle's alternating
buffers (front-end byte history, IF[-1], discriminator output, mixer tail) at either parity and stale data in all of them.

Wherever the receiver is deterministic -- mono always; stereo with the serial PLL (force_generic, pll_mode 1, pll_mode 2) -- a
resumed handle IS the handle that went on: audio, PCM (wrap and saturate) and the state after every block are compared BIT FOR
BIT, no tolerance.  (The default stereo path's parallel PLL re-acquires after set_state; test_state_round_trip keeps its bounds.)
The layout is pinned in both directions against the oracle's own vectors: read in test_gpu_pipeline_params.py, write here, where
the device resumes from a state it never produced.
"""
import numpy as np
import pytest

import _pipeline_cases as pc
from _pipeline_cases import CASES, audio_keys, same_bits
from test_gpu_mfma_exact import FUSED_CASES, MODE_OF_DECIM
from test_gpu_parity import FE_VARIANTS

pytestmark = pytest.mark.gpu

OTHER_SEED = 0xBEEF


def _streams(oracle, p, seed):
    """(b0..b4, two blocks of another stream with other lengths)"""
    n = pc.resume_blocks(p)
    return pc.stream(oracle, p, n, seed), pc.stream(oracle, p, [n[3], n[2]], OTHER_SEED + seed)


def _step(pl, blk, wrap):
    out = pl.process(blk, wrap=wrap)
    return [out[k] for k in audio_keys(pl.channels)] + [out["pcm16"], pl.get_state()]


def check_resume(make, blocks, other, tag, after_first=None):
    """A against the three Bs, for both PCM policies.  make() -> a configured handle; after_first(B): extra check behind B's
    first block after set_state."""
    for wrap in (True, False):
        a = make()
        for blk in blocks[:2]:
            a.process(blk, wrap=wrap)
        st = a.get_state()
        want = [_step(a, blk, wrap) for blk in blocks[2:]]
        a.close()
        for warm in (0, 1, 2):
            b = make()
            for blk in other[:warm]:
                b.process(blk, wrap=wrap)
            if warm:
                assert not np.array_equal(b.get_state(), st)
            b.set_state(st)
            same_bits(b.get_state(), st, f"{tag}: get_state right behind set_state, {warm} blocks before")
            for k, blk in enumerate(blocks[2:]):
                got = _step(b, blk, wrap)
                for name, g, w in zip(audio_keys(b.channels) + ("pcm16", "state"), got, want[k]):
                    same_bits(g, w, f"{tag}: {name}, block {2 + k}, {'wrap' if wrap else 'saturate'}, resumed into a handle that "
                                    f"had processed {warm} blocks")
                if k == 0 and after_first:
                    after_first(b)
            b.close()


# ---- 1. bit-exact resume ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe", FE_VARIANTS)
@pytest.mark.parametrize("rf_taps,au_taps", [(101, 101), (151, 101), (13, 13)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_mono_resume(fmrx, oracle, mode, rf_taps, au_taps, fe):
    p = oracle.mode_params(mode, rf_taps, au_taps, 101)
    blocks, other = _streams(oracle, p, 40 + mode)

    def make():
        pl = fmrx.Pipeline(mode, 1, rf_taps=rf_taps, base_audio_taps=au_taps, max_block_bytes=max(map(len, blocks + other)))
        pl.set_option("fe_variant", fe)
        return pl
    check_resume(make, blocks, other, f"mono mode {mode} {rf_taps}/{au_taps} {fe}")


@pytest.mark.parametrize("T,D,TA,DA", FUSED_CASES)
def test_fused_mono_kernel_right_behind_set_state(fmrx, oracle, T, D, TA, DA):
    """fused_min_audio = 0: the one-kernel path takes IF[-1] and the discriminator tail (prev_in / dhist_end) straight from what
    set_state wrote, in every fused shape."""
    mode = MODE_OF_DECIM[DA]
    p = oracle.mode_params(mode, T, TA, 101)
    assert (p.rf_decim, p.audio_decim) == (D, DA)
    blocks, other = _streams(oracle, p, 60 + mode)

    def make():
        pl = fmrx.Pipeline(mode, 1, rf_taps=T, base_audio_taps=TA, max_block_bytes=max(map(len, blocks + other)))
        pl.set_option("fe_variant", "mfma")
        pl.set_option("fused_min_audio", 0)
        return pl

    def fused_ran(pl):
        with pytest.raises(fmrx.FmrxError):
            pl.read_tap("demod")   # stayed on chip: the fused kernel did the call
    check_resume(make, blocks, other, f"fused mono {T}/{D} {TA}/{DA}", after_first=fused_ran)


def _deterministic(pl, how):
    if how == "force_generic":
        pl.set_force_generic(True)
    else:
        pl.set_option("pll_mode", {"pll_mode 1": 1, "pll_mode 2": 2}[how])


@pytest.mark.parametrize("how", ["force_generic", "pll_mode 1", "pll_mode 2"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_stereo_resume_with_the_serial_pll(fmrx, oracle, mode, how):
    p = oracle.mode_params(mode, 101, 101, 101)
    blocks, other = _streams(oracle, p, 80 + mode)

    def make():
        pl = fmrx.Pipeline(mode, 2, max_block_bytes=max(map(len, blocks + other)))
        _deterministic(pl, how)
        return pl
    check_resume(make, blocks, other, f"stereo mode {mode} {how}")


@pytest.mark.parametrize("how", ["force_generic", "pll_mode 1"])
@pytest.mark.parametrize("name,channels", [("even_stereo_taps", 2), ("hd_from_bandpass", 2), ("ratio_3_8", 1), ("ratio_3_8", 2)])
def test_off_grid_resume(fmrx, oracle, name, channels, how):
    mode, edits, _ = CASES[name]
    p = pc.oracle_params(oracle, mode, edits)
    blocks, other = _streams(oracle, p, 100 + channels)

    def make():
        pl = fmrx.Pipeline(params=pc.device_params(fmrx, mode, edits), channels=channels, max_block_bytes=max(map(len, blocks + other)))
        if channels == 2 or how == "force_generic":
            _deterministic(pl, how)
        return pl
    check_resume(make, blocks, other, f"{name} {channels} ch {how}")


# ---- 3. layout, write direction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_device_resumes_from_the_oracles_state_and_back(fmrx, oracle, mode, channels):
    """The only test in which the device never produced the state it resumes from: the oracle's vectors after b0, b1 go into a
    fresh bit-exact handle, whose b2..b4 must be the oracle's.  And back: the device's state after b0, b1 into a fresh oracle."""
    p = oracle.mode_params(mode, 101, 101, 101)
    blocks, other = _streams(oracle, p, 120 + mode)
    po = oracle.pipeline(mode, channels)
    dev = fmrx.Pipeline(mode, channels, max_block_bytes=max(map(len, blocks)))
    dev.set_force_generic(True)
    for blk in blocks[:2]:
        po.process(blk)
        dev.process(blk)
    st_o, st_d = po.get_state(), dev.get_state()
    same_bits(st_d, st_o, f"mode {mode}, {channels} ch: state after b1")
    for warm in (0, 2):
        pl = fmrx.Pipeline(mode, channels, max_block_bytes=max(map(len, blocks + other)))
        pl.set_force_generic(True)
        for blk in other[:warm]:
            pl.process(blk)
        pl.set_state(st_o)
        back = oracle.pipeline(mode, channels)
        for blk in other[:warm]:
            back.process(blk)
        back.set_state(st_d)
        cont = oracle.pipeline(mode, channels)
        cont.set_state(st_o)
        for k, blk in enumerate(blocks[2:]):
            ref = po.process(blk) if warm == 0 else cont.process(blk)
            out, bk = pl.process(blk), back.process(blk)
            tag = f"mode {mode}, {channels} ch, block {2 + k}, {warm} blocks before"
            for key in audio_keys(channels):
                same_bits(out[key], ref[key], f"device from the oracle's state: {key} {tag}")
                same_bits(bk[key], ref[key], f"oracle from the device's state: {key} {tag}")
            same_bits(pl.read_tap("demod"), ref["demod"], "demod " + tag)
            want = po.get_state() if warm == 0 else cont.get_state()
            same_bits(pl.get_state(), want, "device state " + tag)
            same_bits(back.get_state(), want, "oracle state " + tag)
        pl.close()
    dev.close()


# ---- 4. de-emphasis rides behind the rest -----------------------------------------------------------------------------------
def test_resume_with_deemphasis_mode2_stereo(fmrx, oracle):
    p = oracle.mode_params(2, 101, 101, 101)
    blocks, other = _streams(oracle, p, 140)

    def make():
        pl = fmrx.Pipeline(2, 2, max_block_bytes=max(map(len, blocks + other)))
        pl.set_option("pll_mode", 1)
        n = len(pl.get_state())
        pl.set_deemphasis(50.0)
        assert len(pl.get_state()) == n + 4 == pc.state_size(p, 2) + 4   # {x_prev, y_prev} per audio channel
        return pl
    check_resume(make, blocks, other, "mode 2 stereo, de-emphasis 50 us, pll_mode 1")
    # the four floats are live: after two blocks they are the filter's memory, not zeros
    pl = make()
    for blk in blocks[:2]:
        pl.process(blk)
    assert np.all(pl.get_state()[-4:] != 0)
    pl.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_set_state_refusals_leave_the_handle_alone(fmrx, oracle, channels):
    p = oracle.mode_params(0, 101, 101, 101)
    blocks, other = _streams(oracle, p, 160)
    mk = lambda ch=channels: fmrx.Pipeline(0, ch, max_block_bytes=max(map(len, blocks + other)))
    a, b = mk(), mk()
    for h in (a, b):
        h.set_force_generic(True)
        h.process(blocks[0])
    st = a.get_state()
    n = len(st)
    Tr, Ha, St1 = 100, 100, 100
    bad = []
    bad.append(("one float short", st[:-1]))
    bad.append(("one float long", np.concatenate([st, st[:1]])))
    bad.append(("the other channel count's state", mk(3 - channels).get_state()))
    for where, v in ((0, 0.5 / 128), (Tr - 1, 1.0), (2 * Tr - 1, -1.5), (Tr, np.nan)):   # I_state / Q_state: not (u8 - 128) / 128
        s = st.copy()
        s[where] = v
        bad.append((f"front-end state [{where}] = {v}", s))
    if channels == 2:
        o = 2 * Tr + 2 + Ha                         # state_stereo; state_carrier behind it; state_allpass at the end
        s = st.copy(); s[o + St1 + 7] += 1.0
        bad.append(("state_carrier is not state_stereo", s))
        s = st.copy(); s[n - 6 - 1] += 1.0
        bad.append(("state_allpass is not the tail of state_stereo", s))
        s = st.copy(); s[2 * Tr + 2 + Ha - 1] += 1.0
        bad.append(("state_mono is not the window of state_stereo in front of the all-pass delay", s))
    for why, s in bad:
        with pytest.raises(fmrx.FmrxError) as e:
            b.set_state(s)
        assert e.value.code == fmrx.EINVAL, why
        same_bits(b.get_state(), st, f"handle unchanged after a refused state ({why})")
    with pytest.raises(fmrx.FmrxError):
        fmrx._check(fmrx.lib.fmrx_pipeline_get_state(b._h, np.zeros(n - 1, np.float32), n - 1))
    for blk in blocks[1:3]:
        oa, ob = a.process(blk), b.process(blk)
        for key in audio_keys(channels):
            same_bits(oa[key], ob[key], "after the refusals")
    # the extreme byte values are states: -1 = (0 - 128) / 128 and 127 / 128
    s = st.copy(); s[0], s[1] = -1.0, 127 / 128
    b.set_state(s)
    same_bits(b.get_state(), s)
