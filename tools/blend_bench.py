"""Stereo blend / soft mute (fmrx_blend_*): device time of one pass behind a fast stereo bank of mode 0 and its meters, against
the number of channels.

    python3 tools/blend_bench.py [--channels 192,4096,65536] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, one 192 000-byte block per channel (1 920 audio samples per row), random bytes in the
slots, from device events around every call after the warm-up, the median of `calls` calls.  The bank's call and the meters'
run in front of every timed blend call, outside its pair of events, as in the loop the stage is for.
  blend_ms      fmrx_blend_process_dev out of place with float and PCM output: the control kernel (one lane per channel)
                and the apply kernel (8 bytes in, 8 out and 4 of PCM per stereo sample)
  inplace_ms, f32_ms, pcm_ms   the same call in place, and with only the float / only the PCM output
  copy_ms       hipMemcpyAsync, device to device, of as many bytes as blend_ms reads plus writes (half of them read, half
                written by the copy): the yardstick of a pass that only moves its bytes
  GB_s          bytes read plus written, N * 1 920 * 20, over blend_ms
  bank_ms       fmrx_channels_process_dev of the same bank, and blend_ms relative to it"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _bench_util import copy_call, median_ms  # noqa: E402

BLOCK_BYTES = 192000


def time_config(fmrx, torch, N, calls, warmup):
    bank = fmrx.Channels(0, N, audio_channels=2, exact=False, block_bytes=BLOCK_BYTES)
    meters = fmrx.Meters.for_bank(bank)
    blend = fmrx.Blend.for_bank(bank, meters)
    n = bank.n_audio
    g = torch.Generator(device="cuda").manual_seed(N)
    d_iq = torch.randint(0, 256, (N * BLOCK_BYTES,), dtype=torch.uint8, device="cuda", generator=g)
    d_audio = torch.zeros(N * 2 * n, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(N * 2 * n, dtype=torch.float32, device="cuda")
    d_bank_pcm = torch.zeros(N * 2 * n, dtype=torch.int16, device="cuda")
    d_pcm = torch.zeros(N * 2 * n, dtype=torch.int16, device="cuda")
    moved = N * n * 20                                   # 8 in + 8 out + 4 PCM per stereo sample
    d_src = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    bank.load_dev(d_iq.data_ptr(), stream=s)
    del d_iq
    run_bank = lambda: bank.process_dev(d_audio.data_ptr(), d_bank_pcm.data_ptr(), stream=s)

    def front():
        run_bank()
        meters.process_bank(stream=s)

    bank_ms = median_ms(torch, stream, run_bank, calls, warmup)
    a, o, p = d_audio.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr()
    both = median_ms(torch, stream, lambda: blend.process_bank(a, o, p, stream=s), calls, warmup, front)
    inplace = median_ms(torch, stream, lambda: blend.process_bank(a, a, p, stream=s), calls, warmup, front)
    f32 = median_ms(torch, stream, lambda: blend.process_bank(a, o, None, stream=s), calls, warmup, front)
    pcm = median_ms(torch, stream, lambda: blend.process_bank(a, None, p, stream=s), calls, warmup, front)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), d_src.data_ptr(), moved // 2, s), calls, warmup, front)
    status = blend.status()
    res = dict(channels=N, block_bytes=BLOCK_BYTES, n_audio=n, calls=calls, blend_ms=both[0], blend_ms_min=both[1], blend_ms_max=both[2],
               inplace_ms=inplace[0], f32_ms=f32[0], pcm_ms=pcm[0], copy_ms=copy[0], copy_ms_min=copy[1], moved_bytes=float(moved),
               GB_s=moved / (both[0] * 1e-3) / 1e9, copy_GB_s=moved / (copy[0] * 1e-3) / 1e9, blend_over_copy=both[0] / copy[0],
               bank_ms=bank_ms[0], blend_over_bank=both[0] / bank_ms[0], lamps_on=int(status["lamp"].sum()))
    for x in (blend, meters, bank):
        x.close()
    del d_audio, d_out, d_pcm, d_bank_pcm, d_src, d_dst
    torch.cuda.empty_cache()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="192,4096,65536")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("blend_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "configs": []}
    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d}: blend {r['blend_ms']:8.4f} ms/call (min {r['blend_ms_min']:.4f}, max {r['blend_ms_max']:.4f}; in place {r['inplace_ms']:.4f}, "
              f"float only {r['f32_ms']:.4f}, PCM only {r['pcm_ms']:.4f}), {r['GB_s']:7.1f} GB/s; copy of the same bytes {r['copy_ms']:.4f} ms "
              f"({r['copy_GB_s']:.1f} GB/s), blend / copy = {r['blend_over_copy']:.3f}; bank {r['bank_ms']:.3f} ms/call, blend / bank = "
              f"{r['blend_over_bank']:.4f}", flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
