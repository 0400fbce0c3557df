"""The front of the chain that the *_bank GPU tests of the meters and their stages share: the wide capture of three RDS stations
over noise (tests/_meters_capture.py) -> tuner, 8 channels set from its channel list -> a receiver bank of mode 0, on one stream.
A test opens it, makes its own stages behind the bank, and walks the capture's calls:

    with bank_chain(fmrx, oracle) as ch:
        meters = fmrx.Meters.for_bank(ch.bank)
        for i in ch.calls():                       # call i went through the tuner and the bank on ch.s
            meters.process_bank(stream=ch.s)
            ...
        ch.stream.synchronize()
        meters.close()
"""
import contextlib
import types

import _meters_capture as MC
import _tuner_capture as TC

N = 8


@contextlib.contextmanager
def bank_chain(fmrx, oracle, fused_mono=False, audio_channels=2, exact=False):
    """-> torch, tuner, bank, ac, n (the bank's audio channels and samples per row and call), d_audio float32 [N, ac, n] (what the
    bank writes), stream and s (its handle), first and pitch (the bank's input layout), calls().  fused_mono: the default bank
    (mono, the fused kernel), whatever the other two say.  Tuner and bank are closed on the way out."""
    import torch
    c = TC.RDS
    R, bb = c["R"], MC.BYTES_PER_CALL
    h = oracle.impulse_response_lpf(c["Fs_w"], c["cutoff"], c["T"])
    n_wide = bb // 2 * R
    tuner = fmrx.Tuner(R, h, N, n_wide)
    for k, (f, g) in enumerate(MC.channels()):
        tuner.set_channel(k, f, c["Fs_w"], g)
    if fused_mono:
        bank = fmrx.Channels(0, N, block_bytes=bb)
    else:
        bank = fmrx.Channels(0, N, audio_channels=audio_channels, exact=exact, block_bytes=bb)
    ac, n = bank.audio_channels, bank.n_audio
    d_wide = torch.from_numpy(MC.capture()).cuda()
    d_audio = torch.zeros((N, ac, n), dtype=torch.float32, device="cuda")
    d_bank_pcm = torch.zeros((N, n, ac), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    first, pitch = bank.input_layout()

    def calls():
        torch.cuda.synchronize()          # the buffers, the caller's included, are filled before the stream touches them
        for i in range(MC.CALLS):
            tuner.process_dev(d_wide.data_ptr() + 2 * n_wide * i, n_wide, first, pitch, stream=stream.cuda_stream)
            bank.process_dev(d_audio.data_ptr(), d_bank_pcm.data_ptr(), stream=stream.cuda_stream)
            yield i

    try:
        yield types.SimpleNamespace(torch=torch, tuner=tuner, bank=bank, ac=ac, n=n, d_audio=d_audio, stream=stream, s=stream.cuda_stream,
                                    first=first, pitch=pitch, calls=calls)
    finally:
        tuner.close()
        bank.close()
