"""De-emphasis filter (kernels_deemph.hip): device time of the kernels, of the mode-0 mono step with it off and on, and of the
fast stereo bank with it off and on.

    python3 tools/deemph_bench.py [--what kernels,step,bank] [--n 1048576] [--shapes 256:256,128:128,...] [--blocks 1024]
                                  [--bank-channels 4096,65536] [--tau 75] [--calls 20] [--warmup 3] [--json out.json]

Every figure: device events around each call on one stream, the median of `calls` calls after `warmup` calls.
  kernels  rows 1 and 2 of n samples (the fixed `audio` input of the tests, tiled), fmrx_deemph_dev: the segment kernel + verify
           per lane shape (warm-up:segment), against the one-lane-per-row serial kernel (option deemph_mode = 1); bytes moved =
           one read of x and one write of y, 8 bytes per sample, against the HBM peak (8 TB/s, the figure DESIGN.md uses)
  step     fmrx_pipeline_process_dev, mode 0 mono, `blocks` blocks of 1 024 000 samples per call, PCM out (bench.py's shape and
           outputs): de-emphasis off, on, and the misses per call
  bank     the fast stereo bank (mode 0), one reference-size block per channel and call, PCM out: off and on
--what step --off-only: the off leg alone (one line: for interleaved process pairs against another build's tree)."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.environ.get("FMRX_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # FMRX_TREE: another build's tree
sys.path[:0] = [ROOT]

HBM_PEAK = 8.0e12
BLOCK_BYTES = 102400          # a reference-size block (bank)
STEP_BLOCK_BYTES = 2048000    # bench.py's block: 1 024 000 complex samples


def event_ms(torch, stream, fn, calls, warmup):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(ms_median=statistics.median(ms), ms_min=ms[0], ms_max=ms[-1])


def audio_rows(rows, n, fs=48000.0):
    """the tests' fixed `audio` input (tests/_deemph_model.py: fixed_inputs), 4096 samples, tiled"""
    rng = np.random.default_rng(7)
    t = np.arange(4096) / fs
    a = (0.4 * np.sin(2 * np.pi * 1e3 * t) + 0.2 * np.sin(2 * np.pi * 7e3 * t) + 0.05 * rng.standard_normal(4096)).astype(np.float32)
    return np.stack([np.roll(np.tile(a, (n + 4095) // 4096)[:n], 1000 * r) for r in range(rows)])


def bench_kernels(fmrx, torch, a, out):
    p, b0 = fmrx.deemphasisCoeffs(48000.0, a.tau)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    shapes = [tuple(int(v) for v in sh.split(":")) for sh in a.shapes.split(",")]
    for rows in (1, 2):
        x = torch.from_numpy(audio_rows(rows, a.n)).cuda()
        y = torch.zeros_like(x)
        state = torch.zeros(rows * 2, dtype=torch.float32, device="cuda")
        missed = torch.zeros(1, dtype=torch.int64, device="cuda")
        fn = lambda: fmrx.deemphasis_dev(y.data_ptr(), x.data_ptr(), rows, a.n, a.n, p, b0, state.data_ptr(), missed.data_ptr(), stream=s)
        nbytes = 8.0 * rows * a.n
        for mode, W, L in [(1, 0, 0)] + [(0, W, L) for W, L in shapes]:
            fmrx.set_option("deemph_mode", mode)
            if mode == 0:
                fmrx.set_option("deemph_warmup", W)
                fmrx.set_option("deemph_segment", L)
            torch.cuda.synchronize()
            missed.zero_()
            r = event_ms(torch, stream, fn, a.calls, a.warmup)
            r.update(what="serial kernel" if mode else "segments + verify", rows=rows, n=a.n, W=W, L=L,
                     missed_per_call=int(missed.item()) / (a.calls + a.warmup), GB_s=nbytes / (r["ms_median"] * 1e-3) / 1e9,
                     hbm_share=nbytes / (r["ms_median"] * 1e-3) / HBM_PEAK)
            out["kernels"].append(r)
            print(f"kernels rows={rows} n={a.n} {r['what']:>18s} W={W:4d} L={L:4d}: {r['ms_median']:9.4f} ms (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}), "
                  f"{r['GB_s']:8.1f} GB/s = {100 * r['hbm_share']:.2f} % of HBM peak, missed per call {r['missed_per_call']:.1f}", flush=True)
        for k in ("deemph_mode", "deemph_warmup", "deemph_segment"):
            fmrx.set_option(k, 0 if k == "deemph_mode" else -1)


def step_input(fmrx, blocks):
    """three blocks of one continuous programme (the multiplex repeats every 1 ms, three blocks are 1280 ms), to be tiled"""
    synth = importlib.import_module(fmrx.__name__ + ".synth")
    return synth.synth_fm_u8(3 * STEP_BLOCK_BYTES // 2, 2.4e6, seed=0x3D74 + 10)


def bench_step(fmrx, torch, a, out):
    nb = a.blocks * STEP_BLOCK_BYTES
    d_iq = torch.from_numpy(step_input(fmrx, a.blocks)).cuda().repeat((a.blocks + 2) // 3)[:nb].contiguous()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for tau in (0.0,) if a.off_only else (0.0, a.tau):
        pl = fmrx.Pipeline(0, 1, max_block_bytes=nb)
        if tau:
            pl.set_deemphasis(tau)
        d_pcm = torch.empty(pl.n_audio(nb), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        r = event_ms(torch, stream, lambda: pl.process_dev(d_iq.data_ptr(), nb, None, d_pcm.data_ptr(), wrap=True, stream=s), a.calls, a.warmup)
        r.update(what="mode 0 mono step", blocks=a.blocks, tau_us=tau, msps=nb / 2 / (r["ms_median"] * 1e-3) / 1e6)
        if tau:
            sg, ms = pl.deemph_diagnostics()
            r.update(segments_per_call=sg / (a.calls + a.warmup), missed_per_call=ms / (a.calls + a.warmup))
        out["step"].append(r)
        extra = f", {r['segments_per_call']:.0f} segments and {r['missed_per_call']:.2f} misses per call" if tau else ""
        print(f"step blocks={a.blocks} de-emphasis {'off' if not tau else f'{tau:g} us'}: {r['ms_median']:8.4f} ms (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}), "
              f"{r['msps']:8.1f} MS/s{extra}", flush=True)
        pl.close()
    if len(out["step"]) == 2:
        off, on = out["step"][0]["ms_median"], out["step"][1]["ms_median"]
        print(f"step: de-emphasis costs {on - off:+.4f} ms = {100 * (on - off) / off:+.1f} % of the step", flush=True)


def bench_bank(fmrx, torch, a, out):
    synth = importlib.import_module(fmrx.__name__ + ".synth")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    distinct = 16
    base = torch.stack([torch.from_numpy(synth.synth_fm_u8(BLOCK_BYTES // 2, 2.4e6, seed=0x3D74 + c, start=7919 * c)) for c in range(distinct)]).cuda()
    for nch in [int(v) for v in a.bank_channels.split(",") if v]:
        src = base.repeat((nch + distinct - 1) // distinct, 1)[:nch].contiguous()
        for tau in (0.0, a.tau):
            chs = fmrx.Channels(0, nch, audio_channels=2, exact=False)
            if tau:
                chs.set_deemphasis(tau)
            d_pcm = torch.empty(nch * chs.n_audio * 2, dtype=torch.int16, device="cuda")
            with torch.cuda.stream(stream):
                chs.load_dev(src.data_ptr(), stream=s)
            torch.cuda.synchronize()
            r = event_ms(torch, stream, lambda: chs.process_dev(None, d_pcm.data_ptr(), wrap=True, stream=s), max(a.calls // 2, 5), a.warmup)
            r.update(what="fast stereo bank", channels=nch, tau_us=tau)
            if tau:
                sg, ms = chs.deemph_diagnostics()
                r.update(segments=sg, missed=ms)
            out["bank"].append(r)
            print(f"bank channels={nch:6d} de-emphasis {'off' if not tau else f'{tau:g} us'}: {r['ms_median']:9.4f} ms (min {r['ms_min']:.4f}, max {r['ms_max']:.4f})"
                  + (f", missed {r['missed']} of {r['segments']}" if tau else ""), flush=True)
            chs.close()
            del d_pcm
        del src


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,step,bank")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--shapes", default="256:256,128:128,256:128,128:64,384:256,256:512")
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--bank-channels", default="4096,65536")
    ap.add_argument("--tau", type=float, default=75.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    fmrx = importlib.import_module("software-defined-radio_amd")
    import torch
    if fmrx.device_count() < 1 or not torch.cuda.is_available():
        print("deemph_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    out = {"version": fmrx.version(), "kernels": [], "step": [], "bank": []}
    for what in a.what.split(","):
        {"kernels": bench_kernels, "step": bench_step, "bank": bench_bank}[what](fmrx, torch, a, out)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
