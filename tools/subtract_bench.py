#!/usr/bin/env python3
"""Time of the signal subtraction (thx_subtract) at box 256, 4096 images,
pf 2, r = 127 on one MI355X, for nSym 0 and 3 (D2).  HIP events after warm-up,
median and min-max of the repetitions in one process; one JSON line per
(nSym, outputs), appended to profiles/subtract_bench.jsonl.

Two output sets: "ft" (diffFT alone: the subtraction kernel) and "rl" (diffRL
alone, what save_subtract asks for: the kernel into the workspace, the
Hermitian columns, hipFFT's batched C2R, the scale / centring pass).

Bytes: ori read once + the outputs written once (8 B per stored pixel of every
diffFT plane, 4 B per pixel of every diffRL plane); the projectee gather, the
workspace copy and the C2R's own traffic are left out, so the "rl" rate is an
end-to-end figure, not a share of what the memory system moved.

  python tools/subtract_bench.py [--images 4096] [--box 256] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thunder_amd import ops, subtract, synth  # noqa: E402

HBM_MEASURED_TBPS = 6.29        # float4 copy on MI355X (8.0 TB/s spec)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=4096)
    p.add_argument("--box", type=int, default=256)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "subtract_bench.jsonl"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("subtract_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    N, n, r = a.box, a.images, a.box // 2 - 1
    vol = synth.projectee(synth.blob_volume(N, seed=21, device=dev), 2)
    g = torch.Generator(device=dev).manual_seed(3)
    ori = torch.view_as_complex(torch.randn((n, N, N // 2 + 1, 2), generator=g, device=dev))
    rng = np.random.default_rng(4)
    attr = torch.as_tensor(synth.ctf_attrs(n, seed=6), device=dev)
    quat = torch.as_tensor(synth.uniform_quaternions(n, rng), device=dev)
    trans = torch.as_tensor(rng.standard_normal((n, 2)) * 2, device=dev)
    off = torch.as_tensor(rng.standard_normal((n, 2)), device=dev)
    centre = torch.as_tensor(np.array([12.0, -18.0, 6.0]), device=dev)
    per = N * (N // 2 + 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for sym in (None, "D2"):
        symR = None if sym is None else ops.symmetry(sym)[0]
        copies = 1 + (0 if symR is None else len(symR))
        for outputs in ("ft", "rl"):
            def call():
                subtract.subtract(vol, ori, attr, quat, trans, r, 2, off, None, None, symR, centre,
                                  real=outputs == "rl", model=False, ft=outputs == "ft")
            ms, lo, hi = timed(call, a.warmup, a.reps)
            nbytes = 8.0 * per * n + copies * n * (8.0 * per if outputs == "ft" else 4.0 * N * N)
            rec = {"what": "subtract", "images": n, "box": N, "r": r, "nSym": copies - 1,
                   "outputs": outputs, "ms": ms, "ms_min": lo, "ms_max": hi, "reps": a.reps,
                   "GB": nbytes / 1e9, "GBps": nbytes / ms / 1e6,
                   "fraction_of_measured_hbm": nbytes / ms / 1e6 / (HBM_MEASURED_TBPS * 1e3)}
            print(json.dumps(rec), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
