"""Audio feature frames (fmrx_audio_features_*): device time of one pass over the audio rows of a bank at the 48 kHz preset (win 1200,
hop 480, 201 bins, 80 mels), against the number of channels, and over one long row.

    python3 tools/audio_features_bench.py [--channels 4096,65536] [--n-audio 1920] [--long 1048576] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, rows [N][2][n_audio] of noise at -20 dBFS as a bank would leave them (16-byte aligned), from
device events around every call after the warm-up (which also brings the carried state to its steady 960 samples: 4 frames per
call), the median of `calls` calls:
  features_ms   fmrx_audio_features_process_dev, stereo: the kernel; the results stay on the device
  odd_ms        the rows one float off their alignment (the fetch is 4 bytes per lane either way)
  mono_ms       a mono handle over the first row of every channel's pair: the same matrix work, half the fetch
  spectrum_ms   fmrx_audio_spectrum_process_dev over the same rows, the 23 default bands, on the same visit
  collect_ms    host time of fmrx_audio_features_collect after the device has finished (the copy a consumer on the device avoids)
  copy_ms       hipMemcpyAsync, device to device, of as many bytes as features_ms reads (8 per stereo sample)
  floor_ms      the matrix-issue floor, derived, not measured: per 16 frames 2 ceil(n_bins / 16) row tiles x win / 4 K-steps
                v_mfma_f32_16x16x4_f32 of 32 cycles on one SIMD (26 x 300 at the preset); tiles / 1 024 SIMDs x that at 2.4 GHz
  layout_ms     the same for the kernel's own layout: a wave per pair of bin tiles, 7 waves on the 4 SIMDs of a CU, one workgroup per
                CU: the busiest SIMD issues ceil(waves / 4) x 4 x win / 4 instructions per tile, and a CU holds tiles / 256 of them
--long n: one mono row of n samples (n_channels = 1) the same way: its frames spread over the tiles of one launch; 0 leaves it out."""
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

CUS, SIMDS, CLOCK_HZ, MFMA_CYCLES = 256, 1024, 2.4e9, 32


def floors(p, columns):
    """(floor_ms, layout_ms) of `columns` entries of the (channel, frame) list"""
    tiles = -(-columns // 16)
    bin_tiles = -(-p.n_bins // 16)
    steps = p.win // 4
    floor = tiles / SIMDS * (2 * bin_tiles * steps * MFMA_CYCLES) / CLOCK_HZ * 1e3
    waves = -(-bin_tiles // 2)
    layout = -(-tiles // CUS) * (-(-waves // 4) * 4 * steps * MFMA_CYCLES) / CLOCK_HZ * 1e3
    return floor, layout


def time_config(fmrx, torch, N, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(N)
    d_audio = torch.randn(N * 2 * n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    read = N * 2 * n * 4
    d_dst = torch.zeros(read, dtype=torch.uint8, device="cuda")
    p = fmrx.audioFeaturesPreset(48000.0)
    af = fmrx.AudioFeatures(N, 2, n, p)
    mono = fmrx.AudioFeatures(N, 1, n, p)
    sp = fmrx.AudioSpectrum(N, 2, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    both = median_ms(torch, stream, lambda: af.process_bank(a, stream=s), calls, warmup)
    t0 = time.perf_counter()
    feat, frames = af.collect()
    collect_ms = (time.perf_counter() - t0) * 1e3
    odd = median_ms(torch, stream, lambda: af.process_dev(a + 4, n, n, stream=s), calls, warmup)
    mo = median_ms(torch, stream, lambda: mono.process_dev(a, 2 * n, n, stream=s), calls, warmup)
    spec = median_ms(torch, stream, lambda: sp.process_bank(a, stream=s), calls, warmup)
    copy = median_ms(torch, stream, copy_call(d_dst.data_ptr(), a, read, s), calls, warmup)
    fl, lay = floors(p, N * af.max_frames)
    res = dict(channels=N, n_audio=n, calls=calls, win=p.win, hop=p.hop, n_bins=p.n_bins, n_mels=p.n_mels, max_frames=af.max_frames,
               features_ms=both[0], features_ms_min=both[1], features_ms_max=both[2], odd_ms=odd[0], mono_ms=mo[0], spectrum_ms=spec[0],
               collect_ms=collect_ms, copy_ms=copy[0], read_bytes=float(read), result_bytes=float(feat.nbytes + frames.nbytes), floor_ms=fl, layout_ms=lay,
               features_over_floor=both[0] / fl, features_over_layout=both[0] / lay, features_over_spectrum=both[0] / spec[0],
               x_real_time=n / 48000.0 / (both[0] * 1e-3), frames_ch0=int(frames[0]), frames_min=int(frames.min()), frames_max=int(frames.max()),
               mean_feature_ch0=float(feat[0, :int(frames[0])].mean()))
    for x in (af, mono, sp):
        x.close()
    del d_audio, d_dst
    torch.cuda.empty_cache()
    return res


def time_long(fmrx, torch, n, calls, warmup):
    g = torch.Generator(device="cuda").manual_seed(n)
    d_audio = torch.randn(n + 4, dtype=torch.float32, device="cuda", generator=g) * 0.2
    p = fmrx.audioFeaturesPreset(48000.0)
    af = fmrx.AudioFeatures(1, 1, n, p)
    sp = fmrx.AudioSpectrum(1, 1, n)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, a = stream.cuda_stream, d_audio.data_ptr()
    one = median_ms(torch, stream, lambda: af.process_dev(a, n, n, stream=s), calls, warmup)
    odd = median_ms(torch, stream, lambda: af.process_dev(a + 4, n, n, stream=s), calls, warmup)
    spec = median_ms(torch, stream, lambda: sp.process_dev(a, n, n, stream=s), calls, warmup)
    feat, frames = af.collect()
    fl, lay = floors(p, af.max_frames)
    af.close()
    sp.close()
    return dict(channels=1, audio_channels=1, n_audio=n, calls=calls, max_frames=af.max_frames, features_ms=one[0], features_ms_min=one[1], features_ms_max=one[2],
                odd_ms=odd[0], spectrum_ms=spec[0], floor_ms=fl, layout_ms=lay, features_over_floor=one[0] / fl, features_over_layout=one[0] / lay,
                features_over_spectrum=one[0] / spec[0], x_real_time=n / 48000.0 / (one[0] * 1e-3), frames_ch0=int(frames[0]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536")
    ap.add_argument("--n-audio", type=int, default=1920)
    ap.add_argument("--long", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("audio_features_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "configs": []}

    def save():
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)

    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.n_audio, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d} x 2 x {r['n_audio']}: features {r['features_ms']:8.4f} ms/call (min {r['features_ms_min']:.4f}, max {r['features_ms_max']:.4f}; "
              f"off alignment {r['odd_ms']:.4f}, mono {r['mono_ms']:.4f}); matrix-issue floor {r['floor_ms']:.4f} ms, of the kernel's layout "
              f"{r['layout_ms']:.4f} ms: features / floor = {r['features_over_floor']:.2f}, features / layout = {r['features_over_layout']:.2f}; "
              f"spectrum over the same rows {r['spectrum_ms']:.4f} ms (features / spectrum = {r['features_over_spectrum']:.2f}); "
              f"{r['x_real_time']:.0f} x real time; collect {r['collect_ms']:.3f} ms on the host ({r['result_bytes'] / 1e6:.1f} MB of results); copy of the "
              f"rows' bytes {r['copy_ms']:.4f} ms; frames per channel {r['frames_min']} .. {r['frames_max']} of {r['max_frames']}, mean feature of "
              f"channel 0 {r['mean_feature_ch0']:.4g}", flush=True)
        save()
    if a.long > 0:
        r = time_long(fmrx, torch, a.long, a.calls, a.warmup)
        out["long"] = r
        print(f"one row of {r['n_audio']}: features {r['features_ms']:8.4f} ms/call (min {r['features_ms_min']:.4f}, max {r['features_ms_max']:.4f}; off "
              f"alignment {r['odd_ms']:.4f}); matrix-issue floor {r['floor_ms']:.4f} ms, of the kernel's layout {r['layout_ms']:.4f} ms (features / floor = "
              f"{r['features_over_floor']:.2f}); spectrum over the same row {r['spectrum_ms']:.4f} ms; {r['x_real_time']:.0f} x real time; "
              f"{r['frames_ch0']} frames of {r['max_frames']}", flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
