#!/usr/bin/env python3
"""Are two device-assembly files (hipcc -S --cuda-device-only) the same code?
Compares them function by function and kernel-metadata entry by entry as sets,
so the order in which template instantiations are emitted does not count, with
what depends on that order or on the file's hash made neutral: the function
ordinal in local labels (.LBB12_3, BB12_3 in loop comments) and __hip_cuid_*.
    python tools/asm_funcs_cmp.py A.s B.s      exit status 0: the same code"""
import re
import sys


def split(path):
    txt = open(path).read()
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", txt)
    txt = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|LCPI)\d+", r".\1N", txt)
    txt = re.sub(r"\bBB\d+_", "BBN_", txt)
    head, _, meta = txt.partition("\t.amdgpu_metadata")
    funcs = re.split(r"(?m)^(?=\t\.section\t\.text\.)", head)
    ents = re.split(r"(?m)^(?=  - \.)", meta)
    return funcs[0], sorted(funcs[1:]), ents[0], sorted(ents[1:])


a, b = split(sys.argv[1]), split(sys.argv[2])
differing = sum(x != y for x, y in zip(a[1], b[1])) + abs(len(a[1]) - len(b[1]))
print(f"functions: {len(a[1])} / {len(b[1])}, differing: {differing}; metadata entries: "
      f"{len(a[3])} / {len(b[3])}, equal: {a[3] == b[3]}; rest equal: {a[0] == b[0] and a[2] == b[2]}")
sys.exit(0 if a == b else 1)
