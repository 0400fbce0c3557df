"""Audio meters (fmrx_audio_meters_*): device time of one pass over the audio rows of a bank, against the number of channels.

    python3 tools/audio_meters_bench.py [--channels 4096,16384,65536] [--n-audio 1920] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, rows [N][audio_channels][n_audio] of noise at -20 dBFS as a bank would leave them (16-byte
aligned), from device events around every call after the warm-up, the median of `calls` calls:
  audio_ms      fmrx_audio_meters_process_dev, stereo: the kernel and the copies of its results to the host
  odd_ms        the same rows one float off their alignment: the 4-byte fetch path
  mono_ms       a mono handle over the first row of every channel's pair (half the bytes)
  collect_ms    host time of fmrx_audio_meters_collect after the device has finished (the transposition of the results)
  copy_ms       hipMemcpyAsync, device to device, of as many bytes as audio_ms reads (8 per stereo sample): the stage only reads,
                so half of the copy's traffic is the fair comparison
The high-cut stage at the same shapes is tools/highcut_bench.py --channels ... --long 0, to be run on the same visit."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _bench_util import copy_call, median_ms  # noqa: E402


def time_config(fmrx, torch, N, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(N)
    d_audio = torch.randn(N * 2 * n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    read = N * 2 * n * 4
    d_dst = torch.zeros(read, dtype=torch.uint8, device="cuda")
    am = fmrx.AudioMeters(48000.0, N, 2, n)
    mono = fmrx.AudioMeters(48000.0, N, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    both = median_ms(torch, stream, lambda: am.process_bank(a, stream=s), calls, warmup)
    t0 = time.perf_counter()
    recs, bins = am.collect()
    collect_ms = (time.perf_counter() - t0) * 1e3
    odd = median_ms(torch, stream, lambda: am.process_dev(a + 4, n, n, stream=s), calls, warmup)
    mo = median_ms(torch, stream, lambda: mono.process_dev(a, 2 * n, n, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, read, s), calls, warmup)
    lv = am.derive(recs[0])
    res = dict(channels=N, n_audio=n, calls=calls, audio_ms=both[0], audio_ms_min=both[1], audio_ms_max=both[2], odd_ms=odd[0], mono_ms=mo[0],
               collect_ms=collect_ms, copy_ms=copy[0], read_bytes=float(read), GB_s=read / (both[0] * 1e-3) / 1e9,
               audio_over_copy=both[0] / copy[0], x_real_time=n / 48000.0 / (both[0] * 1e-3), loudness_lkfs_ch0=lv["loudness_lkfs"],
               bins_per_call=int(bins.shape[2]))
    for x in (am, mono):
        x.close()
    del d_audio, d_dst
    torch.cuda.empty_cache()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,16384,65536")
    ap.add_argument("--n-audio", type=int, default=1920)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("audio_meters_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "configs": []}
    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.n_audio, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d} x 2 x {r['n_audio']}: audio meters {r['audio_ms']:8.4f} ms/call (min {r['audio_ms_min']:.4f}, max {r['audio_ms_max']:.4f}; "
              f"4-byte path {r['odd_ms']:.4f}, mono {r['mono_ms']:.4f}), {r['GB_s']:7.1f} GB/s read, {r['x_real_time']:.0f} x real time; collect "
              f"{r['collect_ms']:.3f} ms on the host; copy of the same bytes {r['copy_ms']:.4f} ms (audio meters / copy = {r['audio_over_copy']:.2f}); "
              f"channel 0 reads {r['loudness_lkfs_ch0']:.2f} LKFS", flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
