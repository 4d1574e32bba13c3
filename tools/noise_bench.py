#!/usr/bin/env python3
"""Time of the noise-model update (thx_residual_spectra + thx_sigma_accumulate)
at the bench shape -- 12 500 images, box 256, pf 2, r = 127 -- on one MI355X,
against the expectation step of BENCH_r06.json.  HIP events after warm-up; one
JSON line, appended to profiles/noise_update.jsonl.

Algorithmic bytes: the disc pixels of imgFT and oriFT read once (8 B each);
the projectee gather and the tables are left out (they stay in cache).

  python tools/noise_bench.py [--images 12500] [--box 256] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thunder_amd import noise, synth  # noqa: E402

HBM_MEASURED_TBPS = 6.29        # float4 copy on MI355X (8.0 TB/s spec)
STEP_MS_R06 = 141.78            # BENCH_r06.json ms_per_step


def timed(fn, reps):
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
    return float(np.median(ms))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=12500)
    p.add_argument("--box", type=int, default=256)
    p.add_argument("--groups", type=int, default=1)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_update.jsonl"))
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    N, n, r = a.box, a.images, a.box // 2 - 1
    vol = synth.projectee(synth.blob_volume(N, seed=21, device=dev), 2)
    g = torch.Generator(device=dev).manual_seed(3)
    shape = (n, N, N // 2 + 1, 2)
    img = torch.view_as_complex(torch.randn(shape, generator=g, device=dev))
    ori = torch.view_as_complex(torch.randn(shape, generator=g, device=dev))
    rng = np.random.default_rng(4)
    attr = torch.as_tensor(synth.ctf_attrs(n, seed=6), device=dev)
    quat = torch.as_tensor(synth.uniform_quaternions(n, rng), device=dev)
    trans = torch.as_tensor(rng.standard_normal((n, 2)) * 2, device=dev)
    off = torch.as_tensor(rng.standard_normal((n, 2)), device=dev)
    group = (torch.as_tensor(rng.integers(0, a.groups, n).astype(np.int32), device=dev)
             if a.groups > 1 else None)
    sp = noise.SpectrumPixels(N, r, dev)
    out = {}

    def spectra():
        out["s"] = noise.residual_spectra(vol, img, ori, attr, quat, trans, sp, 2, off)[0]

    def accumulate():
        noise.sigma_accumulate(out["s"], group, a.groups)

    ms_s = timed(spectra, a.reps)
    ms_a = timed(accumulate, a.reps)
    algo = 2.0 * 8.0 * sp.n * n
    rec = {"what": "noise_update", "images": n, "box": N, "r": r, "disc_pixels": sp.n,
           "stored_pixels": N * (N // 2 + 1), "groups": a.groups,
           "ms_residual_spectra": ms_s, "ms_sigma_accumulate": ms_a, "ms": ms_s + ms_a,
           "algorithmic_GB": algo / 1e9,
           "algorithmic_GBps_residual": algo / ms_s / 1e6,
           "fraction_of_measured_hbm": algo / ms_s / 1e6 / (HBM_MEASURED_TBPS * 1e3),
           "ratio_to_step_r06": (ms_s + ms_a) / STEP_MS_R06}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
