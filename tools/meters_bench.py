"""Signal meters (fmrx_meters_*): device time of one pass behind a fast stereo bank of mode 0, against the number of channels.

    python3 tools/meters_bench.py [--channels 192,4096,65536] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, one 192 000-byte block per channel (9 600 discriminator samples: 9 segments and a
remainder), random bytes in the slots, from device events around every call after the warm-up, the median of `calls` calls.
The bank's own call runs in front of every timed meters call, outside its pair of events, as in the loop the stage is for: the
pass follows the bank's call, as it does in use, and does not re-read what it has itself just read.
  meters_ms     fmrx_meters_process_dev: the memset of the accumulators, the RF pass over the slots, the MPX pass over the
                discriminator rows and the two copies of the results to the host
  rf_ms, mpx_ms the same call with only the slots / only the rows given (the other pointer NULL)
  GB_s          the bytes the pass has to read, N * (192 000 + 4 * 9 600), over meters_ms, and its share of the 6.2e12 B/s that the
                project's read-only streaming probe reaches with the default cache policy (6.2 - 7.0)
  bank_ms       fmrx_channels_process_dev of the same bank, and meters_ms relative to it"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _bench_util import median_ms  # noqa: E402

STREAM_PROBE = 6.2e12        # bytes / s
BLOCK_BYTES = 192000


def time_config(fmrx, torch, N, calls, warmup):
    bank = fmrx.Channels(0, N, audio_channels=2, exact=False, block_bytes=BLOCK_BYTES)
    meters = fmrx.Meters.for_bank(bank)
    g = torch.Generator(device="cuda").manual_seed(N)
    d_iq = torch.randint(0, 256, (N * BLOCK_BYTES,), dtype=torch.uint8, device="cuda", generator=g)
    d_audio = torch.zeros(N * 2 * bank.n_audio, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * 2 * bank.n_audio, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    bank.load_dev(d_iq.data_ptr(), stream=s)
    del d_iq
    run_bank = lambda: bank.process_dev(d_audio.data_ptr(), d_pcm.data_ptr(), stream=s)
    bank_ms = median_ms(torch, stream, run_bank, calls, warmup)
    first, pitch = bank.input_layout()
    rows, row_pitch, n_if = bank.demod_layout()
    both = median_ms(torch, stream, lambda: meters.process_dev(first, pitch, BLOCK_BYTES, rows, row_pitch, n_if, stream=s), calls, warmup, run_bank)
    rf = median_ms(torch, stream, lambda: meters.process_dev(first, pitch, BLOCK_BYTES, None, 0, 0, stream=s), calls, warmup, run_bank)
    mpx = median_ms(torch, stream, lambda: meters.process_dev(None, 0, 0, rows, row_pitch, n_if, stream=s), calls, warmup, run_bank)
    meters.collect()
    read_bytes = float(N) * (BLOCK_BYTES + 4 * n_if)
    res = dict(channels=N, block_bytes=BLOCK_BYTES, n_if=n_if, calls=calls, meters_ms=both[0], meters_ms_min=both[1], meters_ms_max=both[2],
               rf_ms=rf[0], mpx_ms=mpx[0], read_bytes=read_bytes, GB_s=read_bytes / (both[0] * 1e-3) / 1e9,
               stream_probe_share=read_bytes / (both[0] * 1e-3) / STREAM_PROBE, rf_GB_s=float(N) * BLOCK_BYTES / (rf[0] * 1e-3) / 1e9,
               mpx_GB_s=float(N) * 4 * n_if / (mpx[0] * 1e-3) / 1e9, bank_ms=bank_ms[0], meters_over_bank=both[0] / bank_ms[0])
    for x in (meters, bank):
        x.close()
    del d_audio, d_pcm
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
        print("meters_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "configs": []}
    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d}: meters {r['meters_ms']:8.4f} ms/call (min {r['meters_ms_min']:.4f}, max {r['meters_ms_max']:.4f}; RF alone {r['rf_ms']:.4f}, "
              f"MPX alone {r['mpx_ms']:.4f}), {r['GB_s']:7.1f} GB/s = {100 * r['stream_probe_share']:.1f} % of the streaming probe "
              f"(RF {r['rf_GB_s']:.1f}, MPX {r['mpx_GB_s']:.1f} GB/s); bank {r['bank_ms']:.3f} ms/call, meters / bank = {r['meters_over_bank']:.4f}",
              flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
