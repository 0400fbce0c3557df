#!/usr/bin/env python3
"""OUT (default build/profb, written by tools/gpu_profile_bench.sh) -> OUT/00_bench_command.txt, OUT/00_bench_command_kernel_stats.csv
and profiles/fe_traffic.json (a copy goes to OUT/fe_traffic.json): the HBM bytes per launch of the fused kernel in the bench command,
with the identity of the build they were counted on."""
import collections, csv, glob, json, shutil, sys

out = sys.argv[1] if len(sys.argv) > 1 else 'build/profb'
L = []
P = L.append
P("rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --no-cpu-baseline --no-side-legs --steps 30 --warmup 5   (MI355X, 1 GPU)")
for f in glob.glob(out + '/trace/**/*kernel_stats.csv', recursive=True):
    shutil.copy(f, out + '/00_bench_command_kernel_stats.csv')
    for i, r in enumerate(csv.DictReader(open(f))):
        if i < 6: P("  {Name:.100s} calls={Calls} avg_ns={AverageNs} min_ns={MinNs} max_ns={MaxNs} pct={Percentage}".format(**r))
for f in glob.glob(out + '/trace/**/*kernel_trace.csv', recursive=True):
    d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(f)) if "mono_fused" in r["Kernel_Name"]]
    if d:
        P(f"== kernel trace, mono_fused_kernel: launches={len(d)} avg_ns(all, incl. the 400 ms settle phase)={sum(d)/len(d):.0f}  "
          f"avg_ns(last 30 = the timed region)={sum(d[-30:])/30:.0f}")
line = [l for l in open(f"{out}/bench_under_rocprof.log") if l.startswith('{')][-1]
bj = json.loads(line)
r = bj["roofline"]
P(f"== bench under rocprof: value {bj['value']} MS/s, ms_per_step {bj['ms_per_step']}, HIP-event avg launch {r['avg_launch_ms']} ms over "
  f"{r['launches_timed']} launches, achieved {r['achieved']} GB/s, frac {r['frac']}, blocks {bj['config']['blocks_per_step']}, "
  f"library {bj['config']['library']['version']}")
tr = {}
for c, d_ in (("FETCH_SIZE", "pmc_fetch"), ("WRITE_SIZE", "pmc_write")):
    v = [float(r["Counter_Value"]) for f in glob.glob(f'{out}/{d_}/**/*counter_collection.csv', recursive=True)
         for r in csv.DictReader(open(f)) if r["Counter_Name"] == c and "mono_fused" in r["Kernel_Name"]]
    if not v:
        sys.exit(f"no {c} counts of mono_fused_kernel under {out}/{d_}")
    tr[c] = sum(v) / len(v)
    P(f"== {c} per dispatch of mono_fused_kernel: {tr[c]:.1f} KB (n={len(v)})")
n = bj["config"]["samples_per_step_per_gpu"]
hbm = int(tr["FETCH_SIZE"] * 1024 * 2 + tr["WRITE_SIZE"] * 1024)
alg = int(n * 2.04)
t = {"blocks": bj["config"]["blocks_per_step"], "output": "s16", "round": "tools/gpu_profile_bench.sh",
     "kernel": "mono_fused_kernel<101,10,101,5>", "lib_src": bj["config"]["library"]["version"].split("src:")[-1],
     "fetch_size_kb": tr["FETCH_SIZE"], "write_size_kb": tr["WRITE_SIZE"], "fetch_correction": 2.0, "hbm_bytes_per_launch": hbm,
     "algorithmic_bytes_per_launch": alg,
     "note": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, per dispatch of `python3 bench.py --no-cpu-baseline --no-side-legs "
             "--steps 5 --warmup 2 --settle-ms 0`; gfx950 FETCH_SIZE counts wide streaming reads at half -> x2; "
             "WRITE_SIZE exact; lib_src = the build (hash of the library's sources) the counters were collected on"}
for dst in (out + '/fe_traffic.json', 'profiles/fe_traffic.json'):
    with open(dst, 'w') as fo:
        json.dump(t, fo, indent=1)
P(f"== HBM traffic per launch: FETCH_SIZE {tr['FETCH_SIZE']:.1f} KB x 2 (gfx950 correction) + WRITE_SIZE {tr['WRITE_SIZE']:.1f} KB = {hbm} B; "
  f"algorithmic {alg} B; ratio {hbm / alg:.3f}")
open(out + '/00_bench_command.txt', 'w').write("\n".join(L) + "\n")
print("\n".join(L))
