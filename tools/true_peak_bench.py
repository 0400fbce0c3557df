"""True-peak meter (fmrx_true_peak_*): device time of one pass over the audio rows of a bank, against the number of channels,
and over one long row.

    python3 tools/true_peak_bench.py [--channels 4096,16384,65536] [--n-audio 1920] [--long 1048576] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, rows [N][audio_channels][n_audio] of noise at -20 dBFS as a bank would leave them (16-byte
aligned), from device events around every call after the warm-up, the median of `calls` calls:
  peak_ms       fmrx_true_peak_process_dev, stereo: the clear of the results, the kernel and the copy of its results to the host
  odd_ms        the same rows one float off their alignment: the 4-byte fetch path
  mono_ms       a mono handle over the first row of every channel's pair (half the bytes)
  collect_ms    host time of fmrx_true_peak_collect after the device has finished
  copy_ms       hipMemcpyAsync, device to device, of as many bytes as peak_ms reads (8 per stereo sample): the stage only reads,
                so half of the copy's traffic is the fair comparison
--long n: one mono row of n samples (n_channels = 1) the same way, against the copy of its bytes; 0 leaves it out.
The audio meters at the same shapes are tools/audio_meters_bench.py --channels ..., to be run on the same visit."""
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
    tp = fmrx.TruePeak(N, 2, n)
    mono = fmrx.TruePeak(N, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    both = median_ms(torch, stream, lambda: tp.process_bank(a, stream=s), calls, warmup)
    t0 = time.perf_counter()
    recs = tp.collect()
    collect_ms = (time.perf_counter() - t0) * 1e3
    odd = median_ms(torch, stream, lambda: tp.process_dev(a + 4, n, n, stream=s), calls, warmup)
    mo = median_ms(torch, stream, lambda: mono.process_dev(a, 2 * n, n, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, read, s), calls, warmup)
    lv = tp.derive(recs[0])
    res = dict(channels=N, n_audio=n, calls=calls, peak_ms=both[0], peak_ms_min=both[1], peak_ms_max=both[2], odd_ms=odd[0], mono_ms=mo[0],
               collect_ms=collect_ms, copy_ms=copy[0], read_bytes=float(read), GB_s=read / (both[0] * 1e-3) / 1e9,
               Gsamples_s=N * 2 * n / (both[0] * 1e-3) / 1e9, peak_over_copy=both[0] / copy[0], x_real_time=n / 48000.0 / (both[0] * 1e-3),
               max_dbtp_ch0=lv["max_dbtp"])
    for x in (tp, mono):
        x.close()
    del d_audio, d_dst
    torch.cuda.empty_cache()
    return res


def time_long(fmrx, torch, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(n)
    d_audio = torch.randn(n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    d_dst = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    tp = fmrx.TruePeak(1, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    one = median_ms(torch, stream, lambda: tp.process_dev(a, n, n, stream=s), calls, warmup)
    odd = median_ms(torch, stream, lambda: tp.process_dev(a + 4, n, n, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, 4 * n, s), calls, warmup)
    lv = tp.derive(tp.collect()[0])
    tp.close()
    return dict(channels=1, audio_channels=1, n_audio=n, calls=calls, peak_ms=one[0], peak_ms_min=one[1], peak_ms_max=one[2], odd_ms=odd[0],
                copy_ms=copy[0], read_bytes=4.0 * n, GB_s=4.0 * n / (one[0] * 1e-3) / 1e9, peak_over_copy=one[0] / copy[0],
                x_real_time=n / 48000.0 / (one[0] * 1e-3), max_dbtp_ch0=lv["max_dbtp"])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,16384,65536")
    ap.add_argument("--n-audio", type=int, default=1920)
    ap.add_argument("--long", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("true_peak_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "tile": fmrx.lib.fmrx_true_peak_tile(), "configs": []}

    def save():
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)

    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.n_audio, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d} x 2 x {r['n_audio']}: true peak {r['peak_ms']:8.4f} ms/call (min {r['peak_ms_min']:.4f}, max {r['peak_ms_max']:.4f}; "
              f"4-byte path {r['odd_ms']:.4f}, mono {r['mono_ms']:.4f}), {r['GB_s']:7.1f} GB/s read, {r['Gsamples_s']:.1f} Gsamples/s, "
              f"{r['x_real_time']:.0f} x real time; collect {r['collect_ms']:.3f} ms on the host; copy of the same bytes {r['copy_ms']:.4f} ms "
              f"(true peak / copy = {r['peak_over_copy']:.2f}); channel 0 reads {r['max_dbtp_ch0']:.2f} dBTP", flush=True)
        save()
    if a.long > 0:
        r = time_long(fmrx, torch, a.long, a.calls, a.warmup)
        out["long"] = r
        print(f"one row of {r['n_audio']}: true peak {r['peak_ms']:8.4f} ms/call (min {r['peak_ms_min']:.4f}, max {r['peak_ms_max']:.4f}; 4-byte path "
              f"{r['odd_ms']:.4f}), {r['GB_s']:7.1f} GB/s read, {r['x_real_time']:.0f} x real time; copy of the same bytes {r['copy_ms']:.4f} ms "
              f"(true peak / copy = {r['peak_over_copy']:.2f}); reads {r['max_dbtp_ch0']:.2f} dBTP", flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
