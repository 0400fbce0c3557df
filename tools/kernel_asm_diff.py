#!/usr/bin/env python3
"""Are the kernels of two device-assembly files the same?  For a change that moves kernels without editing them.
  hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old.hip -o old.s    (likewise new.s)
  python3 tools/kernel_asm_diff.py old.s new.s
Per .amdhsa_kernel symbol: the instruction stream and the .amdhsa_* resource directives, compared after dropping comments,
.file / .ident lines and the __hip_cuid_* symbol and renumbering the function index of local labels (.LBB<n>_).  Exit status 0
when both files hold the same kernel names and every kernel is identical."""
import re
import sys


def kernels(path):
    """name -> (instruction lines, .amdhsa_* lines) of every kernel"""
    text, desc, cur = {}, {}, None
    for raw in open(path):
        s = raw.split(";")[0].strip()              # comments
        if not s or s.startswith((".file", ".ident")) or "__hip_cuid_" in s:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = desc.setdefault(m.group(1), [])
        elif s == ".end_amdhsa_kernel" or s.startswith(".section"):
            cur = None
        elif re.match(r"[A-Za-z_]\w*:$", s):     # a function's entry label; its text ends at the next .section
            cur = text.setdefault(s[:-1], [])
        elif cur is not None:
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {k: (text.get(k), desc[k]) for k in desc}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            print(f"{'missing' if k not in new else 'new':9s} {k}")
            bad += 1
        elif old[k] != new[k] or not old[k][0]:
            print(f"differs   {k}")
            bad += 1
    n_ins = sum(len(t or []) for t, _ in old.values())
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: "
          + (f"{bad} missing, new or different" if bad else f"all identical ({n_ins} lines of instructions and labels each)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
