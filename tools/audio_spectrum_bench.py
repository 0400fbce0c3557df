"""Audio spectrum meter (fmrx_audio_spectrum_*): device time of one pass over the audio rows of a bank, against the number of
channels, and over one long row.

    python3 tools/audio_spectrum_bench.py [--channels 4096,16384,65536] [--n-audio 1920] [--long 1048576] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, rows [N][audio_channels][n_audio] of noise at -20 dBFS as a bank would leave them (16-byte
aligned), from device events around every call after the warm-up, the median of `calls` calls:
  spectrum_ms   fmrx_audio_spectrum_process_dev, stereo, the 23 default bands: the kernel and the copy of its results to the host
  one_band_ms   the same with one band over all bins: the same matrix work and 1/23 of the results, so nearly the kernel alone
  odd_ms        the rows one float off their alignment (the fetch is 4 bytes per lane either way)
  mono_ms       a mono handle over the first row of every channel's pair: two channels share a workgroup
  collect_ms    host time of fmrx_audio_spectrum_collect after the device has finished
  copy_ms       hipMemcpyAsync, device to device, of as many bytes as spectrum_ms reads (8 per stereo sample)
  floor_ms      the matrix-issue floor, derived, not measured: per 16 frames 16 row tiles x 64 K-steps = 1 024 v_mfma_f32_16x16x4_f32
                of 32 cycles on one SIMD; tiles / 1 024 SIMDs x 1 024 x 32 cycles at 2.4 GHz
--long n: one mono row of n samples (n_channels = 1) the same way: the tiled path and its second launch; 0 leaves it out.
The true-peak meter at the same shapes is tools/true_peak_bench.py --channels ..., to be run on the same visit."""
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

SIMDS, CLOCK_HZ, CYCLES_PER_TILE = 1024, 2.4e9, 1024 * 32


def floor_ms(tiles):
    return tiles / SIMDS * CYCLES_PER_TILE / CLOCK_HZ * 1e3


def time_config(fmrx, torch, N, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(N)
    d_audio = torch.randn(N * 2 * n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    read = N * 2 * n * 4
    d_dst = torch.zeros(read, dtype=torch.uint8, device="cuda")
    sp = fmrx.AudioSpectrum(N, 2, n)
    one = fmrx.AudioSpectrum(N, 2, n, edges=(1, 128))
    mono = fmrx.AudioSpectrum(N, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    both = median_ms(torch, stream, lambda: sp.process_bank(a, stream=s), calls, warmup)
    t0 = time.perf_counter()
    recs = sp.collect()
    collect_ms = (time.perf_counter() - t0) * 1e3
    band = median_ms(torch, stream, lambda: one.process_bank(a, stream=s), calls, warmup)
    odd = median_ms(torch, stream, lambda: sp.process_dev(a + 4, n, n, stream=s), calls, warmup)
    mo = median_ms(torch, stream, lambda: mono.process_dev(a, 2 * n, n, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, read, s), calls, warmup)
    lv = sp.derive(recs[0])
    pair = n <= 2048
    tiles = N if pair else 2 * N * -(-((255 + n) // 256) // 16)
    fl = floor_ms(tiles)
    res = dict(channels=N, n_audio=n, calls=calls, spectrum_ms=both[0], spectrum_ms_min=both[1], spectrum_ms_max=both[2], one_band_ms=band[0],
               odd_ms=odd[0], mono_ms=mo[0], collect_ms=collect_ms, copy_ms=copy[0], read_bytes=float(read), result_bytes=float(N * (2 * sp.n_bands * 8 + 4)),
               floor_ms=fl, spectrum_over_floor=both[0] / fl, one_band_over_floor=band[0] / fl, mono_over_floor=mo[0] / floor_ms((N + 1) // 2 if pair else tiles // 2),
               GB_s=read / (both[0] * 1e-3) / 1e9, spectrum_over_copy=both[0] / copy[0], x_real_time=n / 48000.0 / (both[0] * 1e-3),
               frames_ch0=int(recs[0]["frames"]), total_dbfs_ch0=float(lv["total_dbfs"][0]))
    for x in (sp, one, mono):
        x.close()
    del d_audio, d_dst
    torch.cuda.empty_cache()
    return res


def time_long(fmrx, torch, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(n)
    d_audio = torch.randn(n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    d_dst = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    sp = fmrx.AudioSpectrum(1, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    one = median_ms(torch, stream, lambda: sp.process_dev(a, n, n, stream=s), calls, warmup)
    odd = median_ms(torch, stream, lambda: sp.process_dev(a + 4, n, n, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, 4 * n, s), calls, warmup)
    rec = sp.collect()[0]
    lv = sp.derive(rec)
    sp.close()
    fl = floor_ms(-(-((255 + n) // 256) // 16))
    return dict(channels=1, audio_channels=1, n_audio=n, calls=calls, spectrum_ms=one[0], spectrum_ms_min=one[1], spectrum_ms_max=one[2], odd_ms=odd[0],
                copy_ms=copy[0], read_bytes=4.0 * n, floor_ms=fl, spectrum_over_floor=one[0] / fl, GB_s=4.0 * n / (one[0] * 1e-3) / 1e9,
                spectrum_over_copy=one[0] / copy[0], x_real_time=n / 48000.0 / (one[0] * 1e-3), frames_ch0=int(rec["frames"]),
                total_dbfs_ch0=float(lv["total_dbfs"][0]))


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
        print("audio_spectrum_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "frame": fmrx.lib.fmrx_audio_spectrum_frame(), "tile": fmrx.lib.fmrx_audio_spectrum_tile(), "configs": []}

    def save():
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)

    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.n_audio, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d} x 2 x {r['n_audio']}: spectrum {r['spectrum_ms']:8.4f} ms/call (min {r['spectrum_ms_min']:.4f}, max {r['spectrum_ms_max']:.4f}; "
              f"one band {r['one_band_ms']:.4f}, off alignment {r['odd_ms']:.4f}, mono {r['mono_ms']:.4f}); matrix-issue floor {r['floor_ms']:.4f} ms: "
              f"spectrum / floor = {r['spectrum_over_floor']:.2f}, one band / floor = {r['one_band_over_floor']:.2f}, mono / its floor = "
              f"{r['mono_over_floor']:.2f}; {r['GB_s']:7.1f} GB/s read, {r['x_real_time']:.0f} x real time; collect {r['collect_ms']:.3f} ms on the host "
              f"({r['result_bytes'] / 1e6:.1f} MB of results); copy of the rows' bytes {r['copy_ms']:.4f} ms (spectrum / copy = {r['spectrum_over_copy']:.2f}); "
              f"channel 0: {r['frames_ch0']} frames, {r['total_dbfs_ch0']:.2f} dBFS", flush=True)
        save()
    if a.long > 0:
        r = time_long(fmrx, torch, a.long, a.calls, a.warmup)
        out["long"] = r
        print(f"one row of {r['n_audio']}: spectrum {r['spectrum_ms']:8.4f} ms/call (min {r['spectrum_ms_min']:.4f}, max {r['spectrum_ms_max']:.4f}; off "
              f"alignment {r['odd_ms']:.4f}); matrix-issue floor {r['floor_ms']:.4f} ms (spectrum / floor = {r['spectrum_over_floor']:.2f}); "
              f"{r['GB_s']:7.1f} GB/s read, {r['x_real_time']:.0f} x real time; copy of the same bytes {r['copy_ms']:.4f} ms; {r['frames_ch0']} frames, "
              f"{r['total_dbfs_ch0']:.2f} dBFS", flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
