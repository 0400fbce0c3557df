"""HBM traffic of the tuner's matrix kernel from counters-only rocprofv3 runs around tools/tuner_bench.py --once:

    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR/write -- python3 tools/tuner_bench.py --once 192 --calls 3 --warmup 1
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python3 tools/tuner_bench.py --once 192 --calls 3 --warmup 1
    python3 tools/tuner_traffic.py DIR [--channels 192] [--R 8] [--outputs 51200] [--json out.json]

Per dispatch of tuner_mfma_kernel (--kernel tuner_mfma_s16_kernel --sample-bytes 4 for a run with --format s16): WRITE_SIZE (KiB; exact on gfx950, profiles/fe_traffic.json) over the output bytes
2 N n_wide / R, and FETCH_SIZE over the sample-bytes * n_wide input bytes (as counted, and times the 2 that file describes for wide
coalesced reads)."""
import argparse
import csv
import glob
import json
import statistics
import sys


def counter(d, name, kernel):
    v = [float(r["Counter_Value"]) for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True)
         for r in csv.DictReader(open(f)) if r["Counter_Name"] == name and kernel in r["Kernel_Name"]]
    return v


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--channels", type=int, default=192)
    ap.add_argument("--R", type=int, default=8)
    ap.add_argument("--outputs", type=int, default=51200)
    ap.add_argument("--kernel", default="tuner_mfma_kernel")
    ap.add_argument("--sample-bytes", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out_bytes, in_bytes = 2 * a.channels * a.outputs, a.sample_bytes * a.outputs * a.R
    w, f = counter(f"{a.dir}/write", "WRITE_SIZE", a.kernel), counter(f"{a.dir}/fetch", "FETCH_SIZE", a.kernel)
    if not w or not f:
        print(f"tuner_traffic: no {a.kernel} dispatches under {a.dir}", file=sys.stderr)
        return 1
    wb, fb = statistics.median(w) * 1024, statistics.median(f) * 1024
    res = dict(kernel=a.kernel, channels=a.channels, R=a.R, outputs=a.outputs, dispatches=len(w), output_bytes=out_bytes, input_bytes=in_bytes,
               write_bytes=wb, write_ratio=wb / out_bytes, write_ratio_max=max(w) * 1024 / out_bytes, fetch_bytes_counted=fb,
               fetch_ratio_counted=fb / in_bytes, fetch_ratio_x2=2 * fb / in_bytes)
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if res["write_ratio_max"] <= 1.15 else 2


if __name__ == "__main__":
    sys.exit(main())
