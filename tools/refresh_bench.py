#!/usr/bin/env python3
"""Time of the next round's projectee (thx_projectee) on one MI355X at box 256
and 128, pf 2, radial mask: the pruned LDS passes (method 2), the fused pad +
hipFFT fallback (method 1), and the composed path a caller could build without
thx_projectee: a torch element-wise mask x correction (the weight volume
precomputed, outside the timing), the pad written into a zeroed pf N box as
synth.projectee does, then thx_fft3d with method 0.  HIP events after warm-up,
--reps repetitions in one process; one JSON line per box, appended to
profiles/refresh_projectee.jsonl.

The record carries the byte model of each path and the route the decision
rule gives method 0 on this box: the pruned path only if its median beats the
fallback's by more than the fallback's own spread (max - min) over the
repetitions.

  python tools/refresh_bench.py [--boxes 256 128] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thunder_amd import ops, reference  # noqa: E402
from thunder_amd._lib import check, lib  # noqa: E402

HBM_MEASURED_TBPS = 6.29        # float4 copy on MI355X (8.0 TB/s spec)
STEP_MS_R06 = 141.78            # BENCH_r06.json ms_per_step


def timed(fn, reps):
    fn()
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
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": ms}


def signed_axis(n, dev):
    a = torch.arange(n, device=dev)
    return torch.where(a < n // 2, a, a - n).float()


def weight_volume(N, pf, r, edge, dev):
    """mask(|r|) / TIK_RL(|r| / (pf vdim)) on the wrapped N^3 grid (torch, float32)."""
    s = signed_axis(N, dev)
    u = torch.sqrt(s.view(N, 1, 1) ** 2 + s.view(1, N, 1) ** 2 + s.view(1, 1, N) ** 2)
    m = torch.where(u > r + edge, torch.zeros_like(u),
                    torch.where(u >= r, 0.5 + 0.5 * torch.cos((u - r) / edge * np.pi), torch.ones_like(u)))
    x = np.pi * u / (pf * pf * N)
    j0 = torch.where(x == 0, torch.ones_like(x), torch.sin(x) / x.clamp(min=1e-30))
    return (m / (j0 * j0)).contiguous()


def byte_model(N, pf):
    V = pf * N
    H = V // 2 + 1
    src, X, Y, out, pad = 4 * N ** 3, 8 * N * N * H, 8 * N * V * H, 8 * V * V * H, 4 * V ** 3
    return {"pruned_x": src + X, "pruned_y": X + Y, "pruned_z": Y + out,
            "pruned": src + 2 * X + 2 * Y + out,
            # pad written and read, dst written, two in-place column passes over dst
            "fallback": src + 2 * pad + out + 4 * out,
            # torch: weight multiply (2 reads, 1 write), memset, corner copies, then the transform
            "composed": 3 * src + pad + 2 * src + pad + out + 4 * out}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--boxes", type=int, nargs="+", default=[256, 128])
    p.add_argument("--pf", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_projectee.jsonl"))
    a = p.parse_args()
    if a.reps < 5:
        p.error("--reps: at least 5")
    dev = torch.device("cuda", 0)
    L = lib()
    for N in a.boxes:
        pf, V, h = a.pf, a.pf * N, N // 2
        r, edge = N / 2 - 8.0, 6.0
        g = torch.Generator(device=dev).manual_seed(3)
        vol = torch.randn(N, N, N, generator=g, device=dev)
        out = torch.empty(V, V, V // 2 + 1, dtype=torch.complex64, device=dev)
        got = {}

        def run(method):
            got[method] = reference.refresh_projectee(vol, pf, r, edge=edge, method=method, out=out)

        t_pruned = timed(lambda: run("pruned"), a.reps)
        ref = out.clone()
        t_fallback = timed(lambda: run("fallback"), a.reps)
        diff_fb = float((out - ref).abs().max() / ref.abs().max())

        w = weight_volume(N, pf, r, edge, dev)
        pad = torch.empty(V, V, V, device=dev)
        ws = ops.workspace(L.thx_fft3d_workspace(V), dev)
        lo, hi = slice(0, h), slice(N - h, N)
        plo, phi = slice(0, h), slice(V - h, V)

        def composed():
            m = vol * w
            pad.zero_()
            for sz, pz in ((lo, plo), (hi, phi)):
                for sy, py in ((lo, plo), (hi, phi)):
                    for sx, px_ in ((lo, plo), (hi, phi)):
                        pad[pz, py, px_] = m[sz, sy, sx]
            check(L.thx_fft3d(ops._ptr(out), ops._ptr(pad), V, 0, 0, ops._ptr(ws), ws.numel(),
                              ops._stream(dev)), "thx_fft3d")

        t_composed = timed(composed, a.reps)
        diff_c = float((out - ref).abs().max() / ref.abs().max())
        spread = t_fallback["max"] - t_fallback["min"]
        route = "pruned" if t_fallback["median"] - t_pruned["median"] > spread else "fallback"
        bm = byte_model(N, pf)
        rec = {"what": "refresh_projectee", "box": N, "pf": pf, "vdim": V, "mask_radius": r,
               "edge": edge, "reps": a.reps,
               "ms_pruned": t_pruned, "ms_fallback": t_fallback, "ms_composed": t_composed,
               "fallback_spread_ms": spread, "route_method0": route,
               "pruned_over_composed": t_pruned["median"] / t_composed["median"],
               "pruned_over_fallback": t_pruned["median"] / t_fallback["median"],
               "model_GB": {k: v / 1e9 for k, v in bm.items()},
               "model_ms_at_measured_hbm": {k: bm[k] / (HBM_MEASURED_TBPS * 1e9)
                                            for k in ("pruned", "fallback", "composed")},
               "pruned_GBps": bm["pruned"] / t_pruned["median"] / 1e6,
               "fraction_of_measured_hbm": bm["pruned"] / t_pruned["median"] / 1e6 / (HBM_MEASURED_TBPS * 1e3),
               "max_rel_diff_fallback_vs_pruned": diff_fb, "max_rel_diff_composed_vs_pruned": diff_c,
               "auto_ms": None, "ratio_to_step_r06": None}
        t_auto = timed(lambda: run("auto"), a.reps)
        rec["auto_ms"] = t_auto["median"]
        if N == 256:
            rec["ratio_to_step_r06"] = t_auto["median"] / STEP_MS_R06
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del vol, out, pad, w, ref
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
