"""The audio feature frames behind a receiver bank, on the bank's stream: the chain of tests/_bank_chain.py (three RDS stations over
noise -> tuner, 8 channels -> a bank of mode 0) with AudioFeatures.for_bank on the rows the bank wrote, two calls, behind the fast
stereo bank and behind the fused mono bank.  Every feature, frame count and the state equal the model fed the collected rows, and
the host walk, bit for bit; the tensor on the device is what collect() returns."""
import numpy as np
import pytest

import _audio_features_model as af
from _bank_chain import N, bank_chain

pytestmark = pytest.mark.gpu

CALLS = 2


def run_chain(fmrx, oracle, fused_mono):
    import torch
    with bank_chain(fmrx, oracle, fused_mono) as ch:
        m = fmrx.AudioFeatures.for_bank(ch.bank)                       # params None: the preset of the bank's audio rate
        g = {k: getattr(m.params, k) for k in af.FIELDS}
        assert (m.n_channels, m.audio_channels, m.n_audio) == (N, ch.ac, ch.n) and g == af.PRESETS[float(ch.bank.params.audio_Fs)]
        feat_ptr, frames_ptr, shape = m.result_dev()
        assert shape == (N, af.max_frames(ch.n, g), g["n_mels"])
        calls = []
        for i in ch.calls():
            m.process_bank(ch.d_audio.data_ptr(), stream=ch.s)
            feat, frames = m.collect()
            ch.stream.synchronize()

            class Wrapped:
                __cuda_array_interface__ = dict(shape=shape, typestr="<f4", data=(feat_ptr, False), version=2)

            on_device = torch.as_tensor(Wrapped(), device="cuda").cpu().numpy()
            calls.append(dict(feat=feat, frames=frames, on_device=on_device, audio=ch.d_audio.cpu().numpy(), state=m.state()))
            if len(calls) == CALLS:
                break
        ch.stream.synchronize()
        info = dict(calls=calls, ac=ch.ac, n=ch.n, g=g)
        m.close()
    return info


@pytest.fixture(scope="module", params=[False, True], ids=["stereo bank", "fused mono bank"])
def chain(request, fmrx, oracle):
    return run_chain(fmrx, oracle, request.param)


def test_1_every_frame_equals_the_model_and_the_host_walk(fmrx, chain):
    ac, g = chain["ac"], chain["g"]
    assert len(chain["calls"]) == CALLS and ac in (1, 2)
    t = fmrx.audioFeaturesTables(g)
    state, st = af.fresh(N), [None] * N
    T = 0
    for k, call in enumerate(chain["calls"]):
        assert call["audio"].shape == (N, ac, chain["n"])
        want, want_frames, state = af.walk(call["audio"], state, g, t)
        assert af.same(call["feat"], want) and np.array_equal(call["frames"], want_frames), k
        assert af.same(call["state"], state), k
        assert call["on_device"].tobytes() == call["feat"].tobytes(), k
        for c in range(N):
            host, F, st[c] = fmrx.audioFeaturesWalk(call["audio"][c], g, st[c])
            assert af.same(call["feat"][c], host) and F == call["frames"][c], (k, c)
        done = af.frames_of(T, g) if T else 0
        T += chain["n"]
        assert (call["frames"] == af.frames_of(T, g) - done).all(), k
        assert np.isfinite(call["feat"]).all() and (call["feat"][:, :call["frames"][0]] >= 0).all(), k
    assert af.frames_of(T, g) > 0
