"""Wideband tuner (fmrx_tuner_*): device time per call against the number of channels and the decimation, and the tuner's
share of the chain capture -> tuner -> exact stereo bank -> RDS bank.

    python3 tools/tuner_bench.py [--channels 16,192,1024,4096] [--R 8] [--also-R 4,10,20] [--outputs 51200] [--calls 20]
                                 [--warmup 3] [--variant mfma|generic] [--format u8|s8|s16] [--chain 192] [--once N]
                                 [--json out.json] [--ratio U/D [--taps T]]

Per configuration (rf_Fs = 2.4 MS/s, Fs_w = R * rf_Fs, T = 8 R taps of tunerLowPass, channels on the 100 kHz raster; one call =
`outputs` output samples per channel), from device events around every call after the warm-up, the median of `calls` calls:
  wide_MS_s     wide samples per second of device time;  x_real_time = signal time covered / device time
  out_GB_s      output bytes 2 N n_wide / R per second, and its share of the HBM peak (8 TB/s, the figure DESIGN.md uses)
  int8_Top_s    useful int8 operations per second: 2 (multiply, add) * 2 T bytes * 2 rows (re, im) * 2 digits = 16 T per
                channel output, and its share of the dense int8 matrix peak (2 x the 2.5 Pop/s BF16 peak); issued_Top_s counts
                what the matrix kernel really multiplies (the K-steps of all 8 phases of a column, zero padding included)
  bound         which roof is nearer: the larger of output bytes / HBM peak and useful operations / int8 peak
--chain N: the three stages of one 192 000-byte bank block (96 000 outputs per channel, 40 ms of signal), each between its
own pair of events on one stream, N channels.  --once N: a single configuration, `calls` calls and nothing else (for a
counters-only profiler run around this script).  --format: the capture's format, for the tables, --chain and --once alike
(s16: 4 bytes per wide sample in, two byte planes against the same operand image, so twice the matrix operations issued per
output; the output bytes and the useful-operation count of the 8-bit formats are kept as the yardstick).
--ratio U/D: a rational tuner (Tuner.rational, rf_Fs = 2.4 MS/s = Fs_w U / D, T = --taps or 8 D taps of tunerLowPassRational)
instead of the integer one, for every N of --channels (or --once N): `outputs` is rounded down to a multiple of U, Tp =
ceil(T / U) taps meet every output, so the useful operations are 16 Tp per channel output.  The integer path is unchanged."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

HBM_PEAK = 8.0e12            # bytes / s
INT8_PEAK = 5.0e15           # dense int8 op / s
RF_FS = 2.4e6


def shape_ksteps(T, R):
    """K-steps (64 bytes) the matrix kernel multiplies per column and channel group: the sum over the 8 phases"""
    front = (2 * (T - 1) + 15) // 16 * 16
    return sum((front + 2 * R * p + 1) // 64 + 1 - (front + 2 * R * p - 2 * (T - 1)) // 64 for p in range(8))


TORCH_DTYPE = {"u8": "uint8", "s8": "int8", "s16": "int16"}


def random_wide(torch, fmt, n_wide, lo, hi, g):
    """2 n_wide random I,Q values of the format on the device; lo / hi as fractions of full scale around zero"""
    full = 32768 if fmt == "s16" else 128
    off = 128 if fmt == "u8" else 0
    return torch.randint(off + int(lo * full), off + int(hi * full), (2 * n_wide,), dtype=getattr(torch, TORCH_DTYPE[fmt]), device="cuda", generator=g)


def make_tuner(fmrx, R, N, n_wide, T=None, fmt="u8"):
    Fs_w = RF_FS * R
    T = T or 8 * R
    h = fmrx.tunerLowPass(Fs_w, R, T)
    t = fmrx.Tuner(R, h, N, n_wide, fmt=fmt)
    slots = int(Fs_w // 100e3) - 1
    for c in range(N):
        t.set_channel(c, ((c % slots) - slots // 2) * 100e3, Fs_w, 2.0)
    return t, T


def time_config(fmrx, torch, R, N, outputs, calls, warmup, fmt="u8"):
    n_wide = outputs * R
    t, T = make_tuner(fmrx, R, N, n_wide, fmt=fmt)
    pitch = (2 * outputs + 15) // 16 * 16
    g = torch.Generator(device="cuda").manual_seed(R * 100003 + N)
    d_wide = random_wide(torch, fmt, n_wide, -1.0, 1.0, g)
    d_out = torch.zeros(N * pitch, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            t.process_dev(d_wide.data_ptr(), n_wide, d_out.data_ptr(), pitch, stream=stream.cuda_stream)
        for a, b in ev:
            a.record(stream)
            t.process_dev(d_wide.data_ptr(), n_wide, d_out.data_ptr(), pitch, stream=stream.cuda_stream)
            b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    med = statistics.median(ms) * 1e-3
    out_bytes = 2.0 * N * outputs
    ops = 16.0 * T * N * outputs
    issued = shape_ksteps(T, R) * (16 * 16 * 64 * 2) * ((N + 3) // 4) * ((outputs + 127) // 128) * (2 if fmt == "s16" else 1)
    t_hbm, t_mm = out_bytes / HBM_PEAK, ops / INT8_PEAK
    res = dict(format=fmt, R=R, T=T, channels=N, outputs=outputs, calls=calls, ms_median=med * 1e3, ms_min=ms[0], ms_max=ms[-1],
               wide_MS_s=n_wide / med / 1e6, x_real_time=(outputs / RF_FS) / med, out_GB_s=out_bytes / med / 1e9,
               hbm_share=out_bytes / med / HBM_PEAK, int8_Top_s=ops / med / 1e12, int8_share=ops / med / INT8_PEAK,
               issued_Top_s=issued / med / 1e12, bound="HBM writes" if t_hbm >= t_mm else "int8 matrix",
               roof_share=max(t_hbm, t_mm) / med)
    t.close()
    del d_wide, d_out
    return res


def time_ratio(fmrx, torch, U, D, N, outputs, calls, warmup, fmt="u8", T=None):
    """one rational configuration: as time_config, channels on the 100 kHz raster of the capture"""
    outputs = outputs // U * U
    n_wide = outputs // U * D
    Fs_w = RF_FS * D / U
    T = T or 8 * D
    Tp = -(-T // U)
    t = fmrx.Tuner.rational(U, D, fmrx.tunerLowPassRational(Fs_w, U, D, T), N, n_wide, fmt=fmt)
    slots = int(Fs_w // 100e3) - 1
    for c in range(N):
        t.set_channel(c, ((c % slots) - slots // 2) * 100e3, Fs_w, 2.0)
    pitch = (2 * outputs + 15) // 16 * 16
    g = torch.Generator(device="cuda").manual_seed(D * 100003 + N)
    d_wide = random_wide(torch, fmt, n_wide, -1.0, 1.0, g)
    d_out = torch.zeros(N * pitch, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            t.process_dev(d_wide.data_ptr(), n_wide, d_out.data_ptr(), pitch, stream=stream.cuda_stream)
        for a, b in ev:
            a.record(stream)
            t.process_dev(d_wide.data_ptr(), n_wide, d_out.data_ptr(), pitch, stream=stream.cuda_stream)
            b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    med = statistics.median(ms) * 1e-3
    out_bytes = 2.0 * N * outputs
    ops = 16.0 * Tp * N * outputs
    res = dict(format=fmt, U=U, D=D, T=T, Tp=Tp, channels=N, outputs=outputs, n_wide=n_wide, calls=calls, ms_median=med * 1e3, ms_min=ms[0],
               ms_max=ms[-1], wide_MS_s=n_wide / med / 1e6, signal_ms=outputs / RF_FS * 1e3, x_real_time=(outputs / RF_FS) / med,
               out_GB_s=out_bytes / med / 1e9, ns_per_out_byte=med * 1e9 / out_bytes, int8_Top_s=ops / med / 1e12)
    t.close()
    del d_wide, d_out
    return res


def time_chain(fmrx, torch, N, calls, warmup, fmt="u8"):
    R, bb = 8, 192000
    outputs = bb // 2
    n_wide = outputs * R
    t, T = make_tuner(fmrx, R, N, n_wide, fmt=fmt)
    bank = fmrx.Channels(0, N, audio_channels=2, exact=True, block_bytes=bb)
    rds = fmrx.RdsBank(0, N, bb // 20)
    rds.set_stations(True)
    g = torch.Generator(device="cuda").manual_seed(7)
    d_wide = random_wide(torch, fmt, n_wide, -0.25, 0.25, g)
    d_audio = torch.zeros(N * 2 * bank.n_audio, dtype=torch.float32, device="cuda")
    d_pcm = torch.zeros(N * 2 * bank.n_audio, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    first, pitch = bank.input_layout()
    rows, rpitch, _ = bank.demod_layout()
    s = stream.cuda_stream
    parts = {"tuner": [], "bank": [], "rds_bank": []}
    for i in range(warmup + calls):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(stream):
            e[0].record(stream)
            t.process_dev(d_wide.data_ptr(), n_wide, first, pitch, stream=s)
            e[1].record(stream)
            bank.process_dev(d_audio.data_ptr(), d_pcm.data_ptr(), stream=s)
            e[2].record(stream)
            rds.process_dev(rows, rpitch, stream=s)
            e[3].record(stream)
        rds.stations()
        if i >= warmup:
            for k, name in enumerate(parts):
                parts[name].append(e[k].elapsed_time(e[k + 1]))
    med = {k: statistics.median(v) for k, v in parts.items()}
    total = sum(med.values())
    for x in (t, bank, rds):
        x.close()
    return dict(format=fmt, channels=N, R=R, T=T, block_bytes=bb, signal_ms=outputs / RF_FS * 1e3, ms=med, total_ms=total,
                tuner_share=med["tuner"] / total)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="16,192,1024,4096")
    ap.add_argument("--R", type=int, default=8)
    ap.add_argument("--also-R", default="4,10,20")
    ap.add_argument("--outputs", type=int, default=51200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="mfma")
    ap.add_argument("--format", default="u8", choices=sorted(TORCH_DTYPE))
    ap.add_argument("--chain", type=int, default=192)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--ratio", default=None, help="U/D: a rational tuner, e.g. 6/25 for a 10 MS/s capture")
    ap.add_argument("--taps", type=int, default=0, help="with --ratio: prototype taps (default 8 D)")
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("tuner_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    fmrx.set_option("tuner_variant", a.variant)
    out = {"version": fmrx.version(), "variant": a.variant, "format": a.format, "configs": []}
    if a.ratio:
        U, D = (int(v) for v in a.ratio.split("/"))
        for N in ([a.once] if a.once else [int(n) for n in a.channels.split(",") if n]):
            r = time_ratio(fmrx, torch, U, D, N, a.outputs, a.calls, a.warmup, a.format, a.taps or None)
            out["configs"].append(r)
            print(f"{a.format:>3s} {a.variant:>7s} {U}/{D} T={r['T']} (Tp={r['Tp']}) N={N:5d}, {r['outputs']} outputs = {r['signal_ms']:.2f} ms of signal: "
                  f"{r['ms_median']:8.4f} ms/call (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}), {r['x_real_time']:8.1f} x real time, "
                  f"{r['wide_MS_s']:9.0f} wide MS/s, out {r['out_GB_s']:7.1f} GB/s, {r['ns_per_out_byte']:.4f} ns per output byte, "
                  f"int8 {r['int8_Top_s']:.1f} Top/s useful", flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    if a.once:
        configs = [(a.R, a.once)]
    else:
        configs = [(a.R, int(n)) for n in a.channels.split(",") if n] + [(int(r), 192) for r in a.also_R.split(",") if r]
    for R, N in configs:
        r = time_config(fmrx, torch, R, N, a.outputs, a.calls, a.warmup, a.format)
        out["configs"].append(r)
        print(f"{a.format:>3s} R={R:2d} T={r['T']:3d} N={N:5d}: {r['ms_median']:8.4f} ms/call (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}), "
              f"{r['wide_MS_s']:9.0f} wide MS/s, {r['x_real_time']:8.1f} x real time, out {r['out_GB_s']:7.1f} GB/s "
              f"({100 * r['hbm_share']:.1f} % of HBM peak), int8 {r['int8_Top_s']:7.1f} Top/s useful ({100 * r['int8_share']:.1f} % of peak; "
              f"issued {r['issued_Top_s']:.1f}), nearer roof: {r['bound']} ({100 * r['roof_share']:.1f} %)", flush=True)
    if a.chain and not a.once:
        c = time_chain(fmrx, torch, a.chain, max(a.calls // 2, 5), a.warmup, a.format)
        out["chain"] = c
        print(f"chain, {a.format}, N={c['channels']}, one {c['block_bytes']}-byte block ({c['signal_ms']:.1f} ms of signal): tuner {c['ms']['tuner']:.3f} ms, "
              f"exact stereo bank {c['ms']['bank']:.3f} ms, RDS bank {c['ms']['rds_bank']:.3f} ms; tuner share {100 * c['tuner_share']:.1f} %", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
