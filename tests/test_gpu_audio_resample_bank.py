"""The audio rate converter behind a receiver bank, on the bank's stream, through AudioResample.for_bank on the rows the bank wrote:
behind a small stereo bank of mode 0 (48 kHz, two channels, the mono mix to 16 kHz), behind the fused mono bank, and behind a
mode-2 bank (44.1 kHz -> 16 kHz), three calls each.  Every sample, count and the state equal the model fed the bank's own audio, and
the host walk, bit for bit; the PCM is the oracle's pack of those samples."""
import numpy as np
import pytest

import _audio_resample_model as ar

pytestmark = pytest.mark.gpu

CALLS = 3
BANKS = {"stereo bank, mode 0": dict(mode=0, n_channels=2, audio_channels=2), "fused mono bank": dict(mode=0, n_channels=3, audio_channels=1),
         "mode 2 bank": dict(mode=2, n_channels=2, audio_channels=2)}


def run_bank(fmrx, oracle, kw):
    import torch
    bank = fmrx.Channels(**kw)
    N, ac, n, bb = bank.n_channels, bank.audio_channels, bank.n_audio, bank.block_bytes
    fs = int(bank.params.audio_Fs)
    m = fmrx.AudioResample.for_bank(bank, want_f32=True, want_pcm=True)        # params None: the bank's rate to 16 kHz mono
    g = {k: getattr(m.params, k) for k in ar.FIELDS}
    assert g == ar.preset(fs, 16000) and (m.n_channels, m.audio_channels, m.n_audio) == (N, ac, n) and m.shape == (N, 1, ar.max_out(n, g))
    iq = np.stack([oracle.synth_fm_u8(bb // 2 * CALLS, rf_Fs=float(bank.params.rf_Fs), seed=0x3D74 + c, start=7919 * c) for c in range(N)])
    d_iq = [torch.from_numpy(np.ascontiguousarray(iq[:, k * bb:(k + 1) * bb])).cuda() for k in range(CALLS)]
    d_audio = torch.zeros((N, ac, n), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    calls = []
    for k in range(CALLS):
        bank.load_dev(d_iq[k].data_ptr(), stream=stream.cuda_stream)
        bank.process_dev(d_audio.data_ptr(), None, stream=stream.cuda_stream)
        m.process_bank(d_audio.data_ptr(), stream=stream.cuda_stream)
        got = m.collect()
        stream.synchronize()
        calls.append(dict(got, audio_in=d_audio.cpu().numpy(), state=m.state()))
    m.close()
    bank.close()
    return dict(calls=calls, g=g, N=N, ac=ac, n=n, fs=fs)


@pytest.fixture(scope="module", params=list(BANKS))
def chain(request, fmrx, oracle):
    return run_bank(fmrx, oracle, BANKS[request.param])


def test_1_every_sample_equals_the_model_and_the_host_walk(fmrx, oracle, chain):
    g, N, n = chain["g"], chain["N"], chain["n"]
    h = fmrx.audioResampleTaps(g)
    state, st = ar.fresh(N), [None] * N
    fed = done = 0
    for k, call in enumerate(chain["calls"]):
        assert call["audio_in"].shape == (N, chain["ac"], n) and np.abs(call["audio_in"]).max() > 0.01
        want, counts, state = ar.walk(call["audio_in"], state, g, h)
        M = want.shape[2]
        assert np.array_equal(call["counts"], counts) and ar.same(call["audio"][:, :, :M], want) and ar.same(call["state"], state), k
        assert np.array_equal(call["pcm16"], oracle.pcm16(call["audio"].reshape(-1), True).reshape(call["pcm16"].shape)), k
        for c in range(N):
            host, cnt, st[c] = fmrx.audioResampleWalk(call["audio_in"][c], g, st[c])
            assert cnt == counts[c] and ar.same(call["audio"][c, :, :M], host) and ar.same(call["state"][c], st[c]), (k, c)
        fed += n
        assert (counts == ar.outputs_of(fed, g, 0) - done).all(), k
        done += int(counts[0])
        assert np.isfinite(call["audio"]).all()
    assert done == ar.max_out(CALLS * n, g) and chain["fs"] in (48000, 44100)
