#!/usr/bin/env python3
"""Times of mask generation (csrc/mask.hip) and the masked FSC
(csrc/fsc_masked.hip) on one MI355X at boxes 256 and 512.  HIP events after
warm-up, median and min-max of the repetitions in one process; one JSON line
per measurement, appended to profiles/mask_fsc.jsonl.

Mask stages (ext 4, ew 6, a blob map thresholded at its 90th percentile):
  threshold                    one kernel: 7 reads (cache-served) + 1 write per voxel
  pack (+ a one-row ball)      extend with ext = 0.5, whose ball is the voxel itself
  extend, soft_edge            pack + ball kernel each
  gen_mask                     the chain
Algorithmic bytes: threshold 8 B / voxel (read + write), pack 4 B / voxel + the
bits, ball 8 B / voxel + the bits.  Row lookups: one per (voxel, (dy, dz) of
the disc dy^2 + dz^2 < L) whose row is inside the box -- the count the kernel's
loops make before the empty-row skip -- over the stage's time, pack included.

masked_fsc (soft sphere of 0.3 N as alphaMask and as coreR): the whole call,
and the eight transforms alone (four inverse, four forward through ops.fft3d,
which synchronises after each, so their share is an upper bound).

Per-kernel times come from a kernel trace of this script (--reps 2), not from
here.

  python tools/mask_fsc_bench.py [--boxes 256 512] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thunder_amd import mask, ops, resolution, synth  # noqa: E402
from thunder_amd._lib import check, lib  # noqa: E402

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


def disc_rows(N, lim2):
    """sum over voxels of the in-box (dy, dz) with dy^2 + dz^2 < lim2"""
    a = 0
    while (a + 1) ** 2 < lim2:
        a += 1
    inside = np.zeros((N, N), np.int64)
    for dz in range(-a, a + 1):
        for dy in range(-a, a + 1):
            if dy * dy + dz * dz < lim2:
                inside[max(0, -dz):N - max(0, dz), max(0, -dy):N - max(0, dy)] += 1
    return int(inside.sum()) * N


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_fsc.jsonl"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mask_fsc_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(rec):
        rec.update(reps=a.reps)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    def rate(nbytes, ms):
        return {"GB": nbytes / 1e9, "GBps": nbytes / ms / 1e6,
                "fraction_of_measured_hbm": nbytes / ms / 1e6 / (HBM_MEASURED_TBPS * 1e3)}
    for N in a.boxes:
        n3 = N ** 3
        bits = N * N * ((N + 63) // 64) * 8
        vol = torch.fft.ifftshift(synth.blob_volume(N, n_blobs=40, seed=3, device=dev)).contiguous()
        thres = float(torch.quantile(vol.flatten()[::max(1, n3 // 1000000)], 0.9))
        m0 = mask.threshold(vol, thres)
        m1 = mask.extend(m0, 4.0)
        stages = [("threshold", lambda: mask.threshold(vol, thres), 8.0 * n3, None),
                  ("pack_one_row", lambda: mask.extend(m0, 0.5), 12.0 * n3 + 2 * bits, 1),
                  ("extend", lambda: mask.extend(m0, 4.0), 12.0 * n3 + 2 * bits, 16),
                  ("soft_edge", lambda: mask.soft_edge(m1, 6.0), 12.0 * n3 + 2 * bits, 36),
                  ("gen_mask", lambda: mask.gen_mask(vol, thres, 4.0, 6.0), None, None)]
        for name, fn, nbytes, lim2 in stages:
            ms, lo, hi = timed(fn, a.warmup, a.reps)
            rec = {"what": "mask", "stage": name, "box": N, "ext": 4.0, "ew": 6.0, "ms": ms,
                   "ms_min": lo, "ms_max": hi, "mask_fraction": float(m0.mean())}
            if nbytes:
                rec.update(rate(nbytes, ms))
            if lim2:
                rows = disc_rows(N, lim2)
                rec.update(row_lookups=rows, row_lookups_per_s=rows / ms * 1e3)
            emit(rec)
        del m0, m1
        # the masked FSC: two noisy halves of the blob map
        g = torch.Generator(device=dev).manual_seed(5)
        halves = [torch.fft.rfftn(vol + 0.05 * float(vol.max()) * torch.randn(
            vol.shape, generator=g, device=dev)).to(torch.complex64).contiguous() for _ in range(2)]
        ax = torch.fft.fftfreq(N, 1.0 / N, device=dev)
        d = torch.sqrt(ax.view(N, 1, 1) ** 2 + ax.view(1, N, 1) ** 2 + ax.view(1, 1, N) ** 2)
        r, ew = 0.3 * N, 6.0
        alpha = torch.where(d > r + ew, 0.0, torch.where(
            d >= r, 0.5 + 0.5 * torch.cos((d - r) / ew * np.pi), 1.0)).float().contiguous()
        del d
        n_shell = N // 2 - 1
        nft = N * N * (N // 2 + 1)
        for branch, kw in (("alphaMask", dict(mask=alpha)), ("coreR", dict(core_radius=r))):
            ms, lo, hi = timed(lambda: resolution.masked_fsc(halves[0], halves[1], n_shell, edge=ew,
                                                             seed=1, method=0, **kw),
                               a.warmup, a.reps)
            emit({"what": "masked_fsc", "branch": branch, "box": N, "n_shell": n_shell, "ms": ms,
                  "ms_min": lo, "ms_max": hi})
        C = halves[0].clone()
        rl = torch.empty(N, N, N, dtype=torch.float32, device=dev)

        ws = ops.workspace(lib().thx_fft3d_workspace(N), dev)

        def eight():
            for _ in range(4):
                for inv in (1, 0):
                    check(lib().thx_fft3d(ops._ptr(C), ops._ptr(rl), N, inv, 0, ops._ptr(ws),
                                          ws.numel(), None), "thx_fft3d")
        ms, lo, hi = timed(eight, 1, a.reps)
        emit({"what": "fft3d_x8", "box": N, "ms": ms, "ms_min": lo, "ms_max": hi,
              "note": "4 C2R + 4 R2C through thx_fft3d, each followed by a stream synchronise"})
        # the streaming kernels' algorithmic bytes, for the kernel trace: shell sums read both
        # maps (16 B / stored voxel), randomise reads and writes one (16 B), multiply reads the
        # map and alpha and writes the map (12 B / voxel; 8 B on the coreR branch)
        emit({"what": "bytes", "box": N, "shell_sums": 16.0 * nft, "random_phase": 16.0 * nft,
              "mask_mul_alpha": 12.0 * n3, "mask_mul_core": 8.0 * n3, "pack": 4.0 * n3 + bits,
              "ball": 8.0 * n3 + bits, "threshold": 8.0 * n3})
        del halves, alpha, C, rl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
