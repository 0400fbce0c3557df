"""Loudness leveller / peak limiter (fmrx_leveller_*): device time of one pass behind the audio meters, against the number of
channels.

    python3 tools/leveller_bench.py [--channels 4096,65536] [--lookahead 64] [--calls 20] [--warmup 3] [--json out.json]

Per channel count, on one stream, stereo rows of 1 920 samples (one call of a bank at 48 kHz): seeded normal noise at -20 dBFS
RMS with every sixteenth channel 20 dB hotter, and a cut of at most 6 dB (max_cut_db; the other parameters are the defaults), so
that the limiter has work in those rows (channels_limited) and none in the others.  The audio meters run once in front; every
timed call reads their sums where they lie.  From device events around every call after the
warm-up, the median of `calls` calls.
  both_ms       fmrx_leveller_process_dev with float and PCM output: the control kernel (one lane per channel) and the apply
                kernel (8 bytes in, 8 out and 4 of PCM per stereo sample; beside them the carried state, 2W - 2 codes and
                2 (W - 1) floats per channel read and written, 2 016 bytes at W = 64 against 38 400: not counted)
  pcm_ms        the same call with only the PCM output, the end of a chain (8 bytes in, 4 out)
  copy_*_ms     hipMemcpyAsync, device to device, of as many bytes as the call reads plus writes (half of them read, half
                written by the copy): the yardstick of a pass that only moves its bytes
  GB_s          bytes read plus written, N * 1 920 * 20 (12), over both_ms (pcm_ms)
tools/blend_bench.py at the same channel counts gives the blend's apply pass, which moves the same rows."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from _bench_util import copy_call, median_ms  # noqa: E402

N_AUDIO = 1920


def time_config(fmrx, torch, N, W, calls, warmup):
    n = N_AUDIO
    am = fmrx.AudioMeters(48000.0, N, 2, n)
    lv = fmrx.Leveller(48000.0, N, 2, n, fmrx.LevellerParams(max_cut_db=6.0), lookahead=W)
    g = torch.Generator(device="cuda").manual_seed(N)
    d_audio = torch.randn((N, 2, n), dtype=torch.float32, device="cuda", generator=g) * 0.2
    d_audio[::16] *= 10.0
    d_out = torch.zeros(N * 2 * n, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * 2 * n, dtype=torch.int16, device="cuda")
    moved = {"both": N * n * 20, "pcm": N * n * 12}
    d_src = torch.zeros(moved["both"] // 2, dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(moved["both"] // 2, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    am.process_bank(d_audio.data_ptr(), stream=s)
    a, o, p = d_audio.data_ptr(), d_out.data_ptr(), d_pcm.data_ptr()
    both = median_ms(torch, stream, lambda: lv.process_dev(am, a, o, p, stream=s), calls, warmup)
    pcm = median_ms(torch, stream, lambda: lv.process_dev(am, a, None, p, stream=s), calls, warmup)
    def copy_of(nbytes):
        return median_ms(torch, stream, copy_call(d_dst.data_ptr(), d_src.data_ptr(), nbytes // 2, s), calls, warmup)

    copy_both, copy_pcm = copy_of(moved["both"]), copy_of(moved["pcm"])
    status = lv.status()
    res = dict(channels=N, n_audio=n, lookahead=W, tile=lv.tile, calls=calls, both_ms=both[0], both_ms_min=both[1], both_ms_max=both[2],
               pcm_ms=pcm[0], pcm_ms_min=pcm[1], pcm_ms_max=pcm[2], copy_both_ms=copy_both[0], copy_both_ms_min=copy_both[1],
               copy_pcm_ms=copy_pcm[0], copy_pcm_ms_min=copy_pcm[1], moved_both_bytes=float(moved["both"]), moved_pcm_bytes=float(moved["pcm"]),
               both_GB_s=moved["both"] / (both[0] * 1e-3) / 1e9, pcm_GB_s=moved["pcm"] / (pcm[0] * 1e-3) / 1e9,
               both_over_copy=both[0] / copy_both[0], pcm_over_copy=pcm[0] / copy_pcm[0],
               channels_limited=int((status["limited"] > 0).sum()), channels_gated=int(status["gated"].sum()))
    for x in (lv, am):
        x.close()
    del d_audio, d_out, d_pcm, d_src, d_dst
    torch.cuda.empty_cache()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="4096,65536")
    ap.add_argument("--lookahead", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("leveller_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "configs": []}
    for N in [int(n) for n in a.channels.split(",") if n]:
        r = time_config(fmrx, torch, N, a.lookahead, a.calls, a.warmup)
        out["configs"].append(r)
        print(f"N={N:6d} W={r['lookahead']}: float + PCM {r['both_ms']:8.4f} ms/call (min {r['both_ms_min']:.4f}, max {r['both_ms_max']:.4f}), "
              f"{r['both_GB_s']:7.1f} GB/s, copy of the same bytes {r['copy_both_ms']:.4f} ms, leveller / copy = {r['both_over_copy']:.3f}; "
              f"PCM only {r['pcm_ms']:8.4f} ms/call (min {r['pcm_ms_min']:.4f}, max {r['pcm_ms_max']:.4f}), {r['pcm_GB_s']:7.1f} GB/s, copy "
              f"{r['copy_pcm_ms']:.4f} ms, leveller / copy = {r['pcm_over_copy']:.3f}; {r['channels_limited']} channels limited, "
              f"{r['channels_gated']} gated", flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
