"""A signed 16-bit capture in front of the receiver banks, on the device: an S16 tuner's process_dev writes the bank's input
slots, the bank's process_dev follows on the same stream, and the audio / PCM equal, bit for bit, what the same kind of bank
produces when it is fed the integer model's bytes from the host.  Then the three-station RDS capture 42 dB further down,
where an 8-bit capture no longer sees it: S16 tuner -> exact stereo bank -> RDS bank with stations on, every station's PI
and PS."""
import numpy as np
import pytest

import _tuner_capture as TC
import _tuner_formats_capture as FC
import _tuner_formats_model as fm

pytestmark = pytest.mark.gpu


def wide_noise_and_carriers_s16(n_wide, offsets_cps, seed):
    """int16 I,Q: a few frequency-modulated carriers of very different levels (cycles per sample given) over noise"""
    rng = np.random.default_rng(seed)
    n = np.arange(n_wide, dtype=np.float64)
    z = (rng.standard_normal(n_wide) + 1j * rng.standard_normal(n_wide)) * 0.0002
    for k, f in enumerate(offsets_cps):
        z += 0.22 * 10.0 ** (-0.75 * k) * np.exp(1j * (2 * np.pi * f * n + 3.0 * np.sin(2 * np.pi * (k + 1) * 7e-6 * n)))
    return fm.quantise(z, fm.S16)


def s16_tuner_into_bank(fmrx, mode, R, N, audio_channels, exact, n_calls=3):
    import torch
    kw = dict(audio_channels=audio_channels, exact=exact)
    dev_bank, host_bank = fmrx.Channels(mode, N, **kw), fmrx.Channels(mode, N, **kw)
    bb, rf_Fs = dev_bank.block_bytes, dev_bank.params.rf_Fs
    Fs_w, T = float(R * rf_Fs), 8 * R
    h = fmrx.tunerLowPass(Fs_w, R, T)
    n_wide = bb // 2 * R
    carriers = (-0.31, 0.07, 0.38, -0.12)
    cps = [carriers[c % 4] + 0.003 * (c // 4) for c in range(N)]
    wide = wide_noise_and_carriers_s16(n_calls * n_wide, carriers, seed=mode * 100 + R)
    tuner, model = fmrx.Tuner(R, h, N, n_wide, fmt="s16"), fm.TunerModel(h, R, N, fm.S16)
    assert tuner.n_out_bytes(n_wide) == bb and tuner.sample_bytes == 4
    for c in range(N):
        gain = 2.5 * 10.0 ** (0.75 * (c % 4)) * (1.0 + 0.1 * (c % 3))          # each carrier brought to the same level
        tuner.set_channel(c, cps[c] * Fs_w, Fs_w, gain)
        model.set_channel_ints(c, *fmrx.Tuner.design(h, Fs_w, cps[c] * Fs_w, gain))
    ac, na = dev_bank.audio_channels, dev_bank.n_audio
    d_wide = torch.from_numpy(wide.view(np.uint8)).cuda()
    d_audio = torch.zeros(N * ac * na, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * ac * na, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = dev_bank.input_layout()
    for i in range(n_calls):
        tuner.process_dev(d_wide.data_ptr() + 4 * n_wide * i, n_wide, first, pitch, stream=stream.cuda_stream)
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


def test_s16_tuner_into_the_fused_mono_bank(fmrx):
    s16_tuner_into_bank(fmrx, 0, 8, 9, 1, False)


def test_s16_tuner_into_an_exact_stereo_bank(fmrx):
    s16_tuner_into_bank(fmrx, 0, 4, 5, 2, True)


def test_three_rds_stations_from_one_int16_capture(fmrx, oracle):
    """the RDS capture with every amplitude divided by 128, as int16 -> S16 tuner (gains x 128) -> exact stereo bank -> RDS
    bank with stations on, all on one stream.  Required: every station's PI and PS right from the 20th call to the last (the
    CPU statement of the path: tests/test_tuner_formats_host.py).  The u8 quantisation of the capture is within +-1 LSB of 128."""
    import torch
    c = TC.RDS
    N, R, calls, bb = 3, c["R"], c["calls"], c["bytes_per_call"]
    wide, u8 = FC.rds_capture_s16(also_u8=True)
    assert np.abs(u8.astype(np.int32) - 128).max() <= 1
    del u8
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    n_wide = bb // 2 * R
    tuner = fmrx.Tuner(R, h, N, n_wide, fmt="s16")
    for k in range(N):
        tuner.set_channel(k, c["offsets"][k], c["Fs_w"], FC.rds_gain_s16(k))
    bank = fmrx.Channels(0, N, audio_channels=2, exact=True, block_bytes=bb)
    rds = fmrx.RdsBank(0, N, bb // 20)
    rds.set_stations(True)
    d_wide = torch.from_numpy(wide.view(np.uint8)).cuda()
    d_audio = torch.zeros(N * 2 * bank.n_audio, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * 2 * bank.n_audio, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = bank.input_layout()
    d_rows, row_pitch, n_if = bank.demod_layout()
    assert n_if == rds.block
    right, clipped = [], np.zeros(N, np.uint64)
    for i in range(calls):
        tuner.process_dev(d_wide.data_ptr() + 4 * n_wide * i, n_wide, first, pitch, stream=stream.cuda_stream)
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
