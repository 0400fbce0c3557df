"""The front of the chain that the *_bank GPU tests of the leveller and the true-peak meter share, on one stream: a fast stereo bank
of mode 0 with 8 channels on the same synthetic programme -> a gain per channel (0.1, 1, 4, 0 = an empty channel, 30, and 0.1, 1,
4 again) -> AudioMeters.for_bank -> Leveller.for_bank.  A test opens it (`with gain_chain(fmrx, CALLS, lookahead=W) as ch`), makes
its own handles behind it, and walks `for i in ch.calls()`: call i went through the bank, the gains and the audio meters on ch.s."""
import contextlib
import importlib
import types

N = 8
GAINS = (0.1, 1.0, 4.0, 0.0, 30.0, 0.1, 1.0, 4.0)
BYTES_PER_CALL = 192000             # 96 000 I/Q samples at 2.4 MS/s: 1 920 audio samples at 48 kHz
EMPTY, HOT = 3, 4


@contextlib.contextmanager
def gain_chain(fmrx, n_calls, lookahead=64):
    """-> torch, bank, ac, n (the bank's audio channels and samples per row and call), am and lv (the audio meters and the
    leveller behind them), d_audio float32 [N, ac, n] (the bank's rows times the gains: what am read), d_out and d_pcm (for lv to
    write), stream and s (its handle), calls().  While calls() runs, the stream is torch's current one.  Leveller, audio meters
    and bank are closed on the way out."""
    import torch
    synth = importlib.import_module(fmrx.__name__ + ".synth")
    iq = synth.synth_fm_u8(n_calls * BYTES_PER_CALL // 2)
    bank = fmrx.Channels(0, N, audio_channels=2, exact=False, block_bytes=BYTES_PER_CALL)
    ac, n = bank.audio_channels, bank.n_audio
    am = fmrx.AudioMeters.for_bank(bank)
    lv = fmrx.Leveller.for_bank(bank, am, lookahead=lookahead)
    d_iq = torch.from_numpy(iq.reshape(n_calls, BYTES_PER_CALL)).cuda()
    d_gain = torch.tensor(GAINS, dtype=torch.float32, device="cuda").reshape(N, 1, 1)
    d_audio = torch.zeros((N, ac, n), dtype=torch.float32, device="cuda")
    d_out = torch.full((N, ac, n), 7.0, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros((N, n, ac), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def calls():
        torch.cuda.synchronize()          # the buffers, the caller's included, are filled before the stream touches them
        with torch.cuda.stream(stream):
            for i in range(n_calls):
                d_block = d_iq[i].expand(N, BYTES_PER_CALL).contiguous()
                bank.load_dev(d_block.data_ptr(), stream=s)
                bank.process_dev(d_audio.data_ptr(), None, stream=s)
                d_audio.mul_(d_gain)                                           # the stations differ in level
                am.process_bank(d_audio.data_ptr(), stream=s)
                yield i

    try:
        yield types.SimpleNamespace(torch=torch, bank=bank, ac=ac, n=n, am=am, lv=lv, d_audio=d_audio, d_out=d_out, d_pcm=d_pcm, stream=stream,
                                    s=s, calls=calls)
    finally:
        for x in (lv, am, bank):
            x.close()
