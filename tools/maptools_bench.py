#!/usr/bin/env python3
"""Times of the map tools (csrc/maptools.hip behind thunder_amd/maptools.py) on one MI355X at
box 256, per entry point: a transform with 1 matrix and one with the 59 elements of I, the
resizes 256 -> 128 and 128 -> 256 (whole chain and the Fourier move alone), 1000 projections
(transforms only, and with the real images) and the radial mask.

The times are HIP events around whole calls after warm-up, median and min-max of the
repetitions in one process.  (The library's thx_event_pairs_* are recorded only by the
expectation driver; these are the same events taken through torch, as in the other tools.)
Beside each time stand the algorithmic bytes, from the shapes:

  transform    the source once and the result once, 8 B per voxel (+4 with add_src); the
               8 nMat taps per voxel inside the ball are gathers that mostly hit in cache and
               are listed as "gather_bytes", not counted in the rate
  ft_resize    every stored voxel of dst written, the common cube read, 8 B each
  resize       src and dst once, 4 B per voxel each (the transforms' traffic is hipFFT's)
  project      the images written (8 B per stored pixel, + 4 B per real pixel); the 8 taps per
               pixel of the disc are "gather_bytes"
  soft_mask    8 B per voxel

Each rate is also given as a fraction of the 6.29 TB/s a float4 copy reaches on this GPU.

  python tools/maptools_bench.py [--box 256] [--reps 7]

appends one JSON line per stage to profiles/maptools_bench.jsonl.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBPS = 6.29        # float4 copy on MI355X (8.0 TB/s spec)


def timed(fn, warmup, reps):
    import torch
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
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--box", type=int, default=256)
    p.add_argument("--projections", type=int, default=1000)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "maptools_bench.jsonl"))
    a = p.parse_args()
    import torch
    from thunder_amd import maptools, ops, reference, synth
    if not torch.cuda.is_available():
        sys.exit("maptools_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    N, H, n = a.box, a.box // 2, a.projections
    vol = torch.fft.ifftshift(synth.blob_volume(N, device=dev)).contiguous()
    small = maptools.resize(vol, H)
    ft = torch.fft.rfftn(vol).to(torch.complex64).contiguous()
    ft_small = torch.fft.rfftn(small).to(torch.complex64).contiguous()
    R = torch.as_tensor(ops.symmetry("I1")[0].reshape(-1, 9), device=dev)
    one = R[:1].contiguous()
    proj = reference.refresh_projectee(vol, pf=2)
    quat = ops.global_sample_set(n, 2, 1.0, 1, dev)[0]
    mats = ops.rotmat(quat)
    r = N // 2 - 1
    ball = 4.0 / 3.0 * np.pi * r ** 3
    nft = lambda b: b * b * (b // 2 + 1)
    disc = np.pi * r * r / 2
    stages = [
        ("transform_1", lambda: maptools.transform(vol, one), 8.0 * N ** 3, 32.0 * ball),
        ("transform_59_add_src", lambda: maptools.transform(vol, R, add_src=True), 12.0 * N ** 3,
         32.0 * ball * 59),
        ("ft_resize_down", lambda: maptools.ft_resize(ft, H), 16.0 * nft(H), 0.0),
        ("ft_resize_up", lambda: maptools.ft_resize(ft_small, N), 8.0 * (nft(N) + nft(H)), 0.0),
        ("resize_down", lambda: maptools.resize(vol, H), 4.0 * (N ** 3 + H ** 3), 0.0),
        ("resize_up", lambda: maptools.resize(small, N), 4.0 * (N ** 3 + H ** 3), 0.0),
        (f"project_{n}_ft", lambda: maptools.project(proj, mats, N, real=False, ft=True),
         8.0 * n * N * (N // 2 + 1), 64.0 * n * disc),
        (f"project_{n}_real", lambda: maptools.project(proj, mats, N),
         n * (8.0 * N * (N // 2 + 1) + 4.0 * N * N), 64.0 * n * disc),
        ("soft_mask", lambda: maptools.soft_mask(vol, 0.35 * N), 8.0 * N ** 3, 0.0)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name, fn, nbytes, gather in stages:
        rec = {"what": "maptools", "stage": name, "box": N, "reps": a.reps, **timed(fn, a.warmup, a.reps),
               "algorithmic_bytes": nbytes, "gather_bytes": gather}
        rec["GBps"] = nbytes / rec["ms"] / 1e6
        rec["fraction_of_measured_hbm"] = rec["GBps"] / (HBM_MEASURED_TBPS * 1e3)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
