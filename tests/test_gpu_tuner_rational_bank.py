"""The rational-rate tuner in front of the receiver banks, on the device: tuner.process_dev writes the bank's input slots
(Channels.input_layout), the bank's process_dev follows on the same stream, and the audio / PCM equal, bit for bit, what the
same kind of bank produces when fmrx_channels_process is fed the rational model's bytes from the host.  Then one 10 MS/s
int16 capture holding three RDS stations -> 6/25 -> exact stereo bank -> RDS bank with stations on: every station's PI and PS."""
import numpy as np
import pytest

import _tuner_formats_model as fm
import _tuner_rational_capture as RC
import _tuner_rational_model as rm

pytestmark = pytest.mark.gpu

FMT_NAMES = {fm.U8: "u8", fm.S8: "s8", fm.S16: "s16"}


def wide_noise_and_carriers(n_wide, offsets_cps, seed, fmt):
    """a few frequency-modulated carriers (cycles per sample given) over noise, quantised to the format"""
    rng = np.random.default_rng(seed)
    n = np.arange(n_wide, dtype=np.float64)
    z = (rng.standard_normal(n_wide) + 1j * rng.standard_normal(n_wide)) * 0.03
    for k, f in enumerate(offsets_cps):
        z += 0.22 * np.exp(1j * (2 * np.pi * f * n + 3.0 * np.sin(2 * np.pi * (k + 1) * 7e-6 * n)))
    return fm.quantise(z, fmt)


def rational_tuner_into_bank(fmrx, mode, U, D, fmt, N, audio_channels, exact, n_calls=3):
    """The bank's block: the largest below 100 000 bytes that is a whole number of the bank's own units, of 16 bytes and of
    8 U output samples -- n_wide is then a multiple of 8 D, so that every call of the capture starts 16-byte aligned."""
    import torch
    kw = dict(audio_channels=audio_channels, exact=exact)
    probe = fmrx.Channels(mode, 1, **kw)
    unit = probe.block_bytes // probe.n_audio              # bytes of input per audio sample: what a block is a multiple of
    probe.close()
    grid = int(np.lcm.reduce([unit, 16, 2 * 8 * U]))
    bb = 100000 // grid * grid
    dev_bank, host_bank = fmrx.Channels(mode, N, block_bytes=bb, **kw), fmrx.Channels(mode, N, block_bytes=bb, **kw)
    assert dev_bank.block_bytes == bb
    rf_Fs = dev_bank.params.rf_Fs
    Fs_w, T = float(rf_Fs) * D / U, 8 * D
    h = fmrx.tunerLowPassRational(Fs_w, U, D, T)
    n_wide = bb // 2 // U * D
    assert n_wide % (8 * D) == 0
    cps = [(-0.31, 0.07, 0.38, -0.12)[c % 4] + 0.003 * (c // 4) for c in range(N)]
    wide = wide_noise_and_carriers(n_calls * n_wide, sorted(set(cps))[:4], mode * 100 + D, fmt)
    tuner, model = fmrx.Tuner.rational(U, D, h, N, n_wide, fmt=FMT_NAMES[fmt]), rm.TunerRationalModel(h, U, D, N, fmt)
    assert tuner.n_out_bytes(n_wide) == dev_bank.block_bytes
    for c in range(N):
        gain = 2.5 * (1.0 + 0.1 * (c % 3))
        tuner.set_channel(c, cps[c] * Fs_w, Fs_w, gain)
        model.set_channel_ints(c, *fmrx.Tuner.design_rational(h, U, Fs_w, cps[c] * Fs_w, gain))
    ac, na = dev_bank.audio_channels, dev_bank.n_audio
    d_wide = torch.from_numpy(wide.view(np.uint8)).cuda()
    d_audio = torch.zeros(N * ac * na, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * ac * na, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = dev_bank.input_layout()
    call_bytes = tuner.sample_bytes * n_wide
    for i in range(n_calls):
        tuner.process_dev(d_wide.data_ptr() + call_bytes * i, n_wide, first, pitch, stream=stream.cuda_stream)
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


def test_6_25_from_10_ms_u8_into_the_fused_mono_bank_mode_0(fmrx):
    rational_tuner_into_bank(fmrx, 0, 6, 25, fm.U8, 9, 1, False)


def test_3_25_from_20_ms_s8_into_an_exact_stereo_bank_mode_0(fmrx):
    rational_tuner_into_bank(fmrx, 0, 3, 25, fm.S8, 5, 2, True)


def test_18_125_from_10_ms_s16_into_a_mode_1_bank(fmrx):
    rational_tuner_into_bank(fmrx, 1, 18, 125, fm.S16, 6, 1, False)


def test_three_rds_stations_from_one_10_ms_int16_capture(fmrx):
    """capture -> 6/25 -> exact stereo bank -> RDS bank with stations on, all on one stream.  Required: every station's PI and PS
    right from call RIGHT_FROM_CALL + 4 = 20 to the last (the CPU statement of the path has them from call 16:
    tests/test_tuner_rational_model_host.py), and no tuned byte clipped."""
    import torch
    c = RC.RDS
    N, U, D, calls, bb = 3, c["U"], c["D"], c["calls"], c["bytes_per_call"]
    wide = RC.rds_capture_10ms_s16()
    h = fmrx.tunerLowPassRational(c["Fs_w"], U, D, c["T"])
    n_wide = RC.N_WIDE_PER_CALL
    tuner = fmrx.Tuner.rational(U, D, h, N, n_wide, fmt="s16")
    assert tuner.n_out_bytes(n_wide) == bb
    for k in range(N):
        tuner.set_channel(k, c["offsets"][k], c["Fs_w"], RC.rds_gain(k))
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
    assert all(s is not None and s <= RC.RIGHT_FROM_CALL + 4 for s in since), \
        f"PI and PS right from call {RC.RIGHT_FROM_CALL + 4} to the last is required; seen: " + report
