"""The wideband tuner in front of the receiver banks, on the device: tuner.process_dev writes the bank's input slots
(Channels.input_layout), the bank's process_dev follows on the same stream, and the audio / PCM equal, bit for bit, what the
same kind of bank produces when fmrx_channels_process is fed the integer model's bytes from the host.  Then one capture
holding three RDS stations -> tuner -> exact stereo bank -> RDS bank with stations on: every station's PI and PS."""
import numpy as np
import pytest

import _tuner_capture as TC
import _tuner_model as tm

pytestmark = pytest.mark.gpu


def wide_noise_and_carriers(n_wide, offsets_cps, seed):
    """u8 I,Q: a few frequency-modulated carriers (cycles per sample given) over noise; realistic enough to exercise the banks"""
    rng = np.random.default_rng(seed)
    n = np.arange(n_wide, dtype=np.float64)
    z = (rng.standard_normal(n_wide) + 1j * rng.standard_normal(n_wide)) * 0.03
    for k, f in enumerate(offsets_cps):
        z += 0.22 * np.exp(1j * (2 * np.pi * f * n + 3.0 * np.sin(2 * np.pi * (k + 1) * 7e-6 * n)))
    iq = np.empty(2 * n_wide, np.uint8)
    iq[0::2] = np.clip(np.floor(128.0 + 127.0 * z.real + 0.5), 0, 255)
    iq[1::2] = np.clip(np.floor(128.0 + 127.0 * z.imag + 0.5), 0, 255)
    return iq


def tuner_into_bank(fmrx, mode, R, N, audio_channels, exact, n_calls=3):
    import torch
    kw = dict(audio_channels=audio_channels, exact=exact)
    dev_bank, host_bank = fmrx.Channels(mode, N, **kw), fmrx.Channels(mode, N, **kw)
    bb, rf_Fs = dev_bank.block_bytes, dev_bank.params.rf_Fs
    Fs_w, T = float(R * rf_Fs), 8 * R
    h = fmrx.tunerLowPass(Fs_w, R, T)
    assert len(h) == T and abs(float(h.sum()) - 1.0) < 0.05
    n_wide = bb // 2 * R
    cps = [(-0.31, 0.07, 0.38, -0.12)[c % 4] + 0.003 * (c // 4) for c in range(N)]
    wide = wide_noise_and_carriers(n_calls * n_wide, sorted(set(cps))[:4], seed=mode * 100 + R)
    tuner, model = fmrx.Tuner(R, h, N, n_wide), tm.TunerModel(h, R, N)
    assert tuner.n_out_bytes(n_wide) == bb
    for c in range(N):
        gain = 2.5 * (1.0 + 0.1 * (c % 3))
        tuner.set_channel(c, cps[c] * Fs_w, Fs_w, gain)
        model.set_channel_ints(c, *fmrx.Tuner.design(h, Fs_w, cps[c] * Fs_w, gain))
    ac, na = dev_bank.audio_channels, dev_bank.n_audio
    d_wide = torch.from_numpy(wide).cuda()
    d_audio = torch.zeros(N * ac * na, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * ac * na, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = dev_bank.input_layout()
    for i in range(n_calls):
        tuner.process_dev(d_wide.data_ptr() + 2 * n_wide * i, n_wide, first, pitch, stream=stream.cuda_stream)
        dev_bank.process_dev(d_audio.data_ptr(), d_pcm.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        tuned = model.process(wide[2 * n_wide * i:2 * n_wide * (i + 1)])
        cl, pw = tuner.levels()
        assert np.array_equal(cl, model.clipped) and np.array_equal(pw, model.power), f"call {i}: levels"
        want = host_bank.process(tuned)
        got_a = d_audio.cpu().numpy().reshape(want["audio"].shape)
        got_p = d_pcm.cpu().numpy().reshape(want["pcm16"].shape)
        assert np.array_equal(got_a.view(np.uint32), want["audio"].view(np.uint32)), f"mode {mode} call {i}: audio"
        assert np.array_equal(got_p, want["pcm16"]), f"mode {mode} call {i}: pcm16"
        assert np.abs(want["audio"]).max() > 0
    for x in (tuner, dev_bank, host_bank):
        x.close()


def test_tuner_into_the_fused_mono_bank_mode_0(fmrx):
    tuner_into_bank(fmrx, 0, 8, 9, 1, False)


def test_tuner_into_an_exact_stereo_bank_mode_0(fmrx):
    tuner_into_bank(fmrx, 0, 4, 5, 2, True)


def test_tuner_into_a_mode_1_bank_decimation_10(fmrx):
    tuner_into_bank(fmrx, 1, 10, 6, 1, False)


def test_tuner_into_a_mode_2_bank(fmrx):
    tuner_into_bank(fmrx, 2, 8, 6, 1, False)


def test_three_rds_stations_from_one_capture(fmrx, oracle):
    """capture -> tuner -> exact stereo bank -> RDS bank with stations on, all on one stream.  Required: every station's PI and
    PS right from the 20th call to the last (the CPU statement of the path has them from the 16th: tests/test_tuner_model_host.py)."""
    import torch
    c = TC.RDS
    N, R, calls, bb = 3, c["R"], c["calls"], c["bytes_per_call"]
    wide = TC.rds_capture()
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    n_wide = bb // 2 * R
    tuner = fmrx.Tuner(R, h, N, n_wide)
    for k in range(N):
        tuner.set_channel(k, c["offsets"][k], c["Fs_w"], TC.rds_gain(k))
    bank = fmrx.Channels(0, N, audio_channels=2, exact=True, block_bytes=bb)
    rds = fmrx.RdsBank(0, N, bb // 20)
    rds.set_stations(True)
    d_wide = torch.from_numpy(wide).cuda()
    d_audio = torch.zeros(N * 2 * bank.n_audio, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * 2 * bank.n_audio, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = bank.input_layout()
    d_rows, row_pitch, n_if = bank.demod_layout()
    assert n_if == rds.block
    right, clipped = [], np.zeros(N, np.uint64)
    for i in range(calls):
        tuner.process_dev(d_wide.data_ptr() + 2 * n_wide * i, n_wide, first, pitch, stream=stream.cuda_stream)
        bank.process_dev(d_audio.data_ptr(), d_pcm.data_ptr(), stream=stream.cuda_stream)
        rds.process_dev(d_rows, row_pitch, stream=stream.cuda_stream)
        st, _ = rds.stations()
        clipped += tuner.levels()[0]
        right.append([st[k]["pi"] == c["pi"][k] and st[k]["ps"] == c["ps"][k] for k in range(N)])
    since = [next((i + 1 for i in range(calls) if all(r[k] for r in right[i:])), None) for k in range(N)]
    report = ", ".join(f"station {k} (PI {c['pi'][k]:04X} '{c['ps'][k]}') from call {since[k]}, {st[k]['good_blocks']} of {st[k]['blocks']} blocks"
                       for k in range(N))
    print("PI and PS right: " + report)
    assert not clipped.any(), f"tuned bytes clipped: {clipped}"
    assert all(s is not None and s <= 20 for s in since), "PI and PS right from the 20th call to the last is required; seen: " + report
