#!/usr/bin/env python3
"""Generate tests/golden/ref_calls.npz from the COMPILED REFERENCE (build container only).

Runs tests/test_oracle_vs_ref.py with the `ref` fixture in recording mode: every
call the tests make to oracle/_ref/libfmref.so (built by oracle/Makefile from
the reference's sources) is answered by that library and its answer stored under
the SHA-256 of the call's name and arguments (tests/_oracle.py, RecordingRef).
Afterwards the same tests run everywhere against the stored answers.  Only data
is written: no reference source.

    python tests/golden/make_golden_ref.py    # needs oracle/_ref/libfmref.so
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, "ref_calls.npz")


def main():
    env = dict(os.environ, FMRX_RECORD_REF=OUT)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        os.path.join(TESTS, "test_oracle_vs_ref.py"), "-k", "not fair_cpu_baseline"], env=env)
    if r.returncode != 0:
        sys.exit(r.returncode)
    print(f"ref_calls.npz: {os.path.getsize(OUT) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
