#!/usr/bin/env python3
"""Times of post-processing (csrc/postprocess.hip behind
thunder_amd/postprocess.py) on one MI355X at boxes 256 and 512, per stage:
the FSC, pass 1 (the Guinier sums), the fit, pass 2 (merge x FSC weight x
B-factor x low pass), the inverse transform and the final multiply.

Two kinds of numbers, named for what they are:

  events   HIP events around whole calls after warm-up, median and min-max of
           the repetitions in one process: the chain (estimating, with a given
           B-factor, with and without the average), the FSC alone, and the
           stage entry points alone.  "pass1_and_fit_by_difference" and
           "average_by_difference" are differences of two such medians.
  kernels  per-kernel times inside the chain, from a kernel trace
           (rocprofv3 --kernel-trace --stats) of `--trace-run`, a run of its
           own that calls nothing but the chain without the average, so every
           kernel of this file appears once per call.  `--fold` puts the
           trace's averages next to the events.

Algorithmic bytes come from the shapes: the shell-sum kernels read 16 B per
stored voxel of the shells they sum (rows end where the shell passes the
limit), pass 2 reads both halves and writes one map (24 B per stored voxel),
the final multiply reads the map and the mask and writes the map (12 B per
voxel).  Each is given over its time as a fraction of the 6.29 TB/s a float4
copy reaches on this GPU (8.0 TB/s spec).

  python tools/postprocess_bench.py [--boxes 256 512] [--reps 7] --events events.jsonl
  rocprofv3 --kernel-trace --stats --output-format csv -d trace256 -o run -- \\
      python tools/postprocess_bench.py --boxes 256 --trace-run
  python tools/postprocess_bench.py --fold events.jsonl --kernel-stats 256=trace256 512=trace512

--fold needs no GPU and appends one JSON line per box to
profiles/postprocess_bench.jsonl.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBPS = 6.29        # float4 copy on MI355X (8.0 TB/s spec)
PIXEL_SIZE, SEED, GIVEN_B = 1.0, 1, -50.0
KERNELS = ("k_shell_partial", "k_shell_final", "k_random_phase", "k_hermitian_planes", "k_mask_mul",
           "k_fsc_combine", "k_pp_prepare", "k_guinier_partial", "k_guinier_fit", "k_ft_stream",
           "k_pp_scale_mask")


def stored_below(N, R):
    """stored voxels whose shell rint|(i, j, k)| is below R"""
    ax = np.fft.fftfreq(N, 1.0 / N)
    c2 = ax[:, None] ** 2 + ax[None, :] ** 2
    lim = (R - 0.5) ** 2 - c2           # i^2 < lim
    n = np.where(lim > 0, np.minimum(np.ceil(np.sqrt(np.maximum(lim, 0))), N // 2 + 1), 0)
    return int(n.sum())


def rate(nbytes, ms):
    return {"GB": nbytes / 1e9, "GBps": nbytes / ms / 1e6,
            "fraction_of_measured_hbm": nbytes / ms / 1e6 / (HBM_MEASURED_TBPS * 1e3)}


def inputs(N, dev):
    """Two halves made in Fourier space, so that no transform of the set-up shows in a kernel
    trace: a common complex Gaussian field under the envelope exp(-20 (u/N)^2) (a B-factor of
    80 A^2 at 1 A / voxel) plus independent complex white noise per half whose power is six
    times the signal's at u = N/3, where the FSC therefore passes 1/7 = 0.143; a soft sphere of
    radius 0.3 N as the mask."""
    import torch
    g = torch.Generator(device=dev).manual_seed(5)
    ax = torch.fft.fftfreq(N, 1.0 / N, device=dev)
    u2 = (ax.view(N, 1, 1) ** 2 + ax.view(1, N, 1) ** 2 + ax[:N // 2 + 1].abs().view(1, 1, -1) ** 2)
    u2[:, :, N // 2] = ax.view(N, 1) ** 2 + ax.view(1, N) ** 2 + (N / 2) ** 2
    env = torch.exp(-20.0 * u2 / (N * N))
    sigma = float(np.sqrt(6.0) * np.exp(-20.0 / 9.0))
    shape = (N, N, N // 2 + 1)
    field = lambda: torch.complex(torch.randn(shape, generator=g, device=dev),
                                  torch.randn(shape, generator=g, device=dev))
    signal = field() * env
    halves = [(signal + sigma * field()).to(torch.complex64).contiguous() for _ in range(2)]
    d = torch.sqrt(ax.view(N, 1, 1) ** 2 + ax.view(1, N, 1) ** 2 + ax.view(1, 1, N) ** 2)
    r, ew = 0.3 * N, 6.0
    alpha = torch.where(d > r + ew, 0.0, torch.where(
        d >= r, 0.5 + 0.5 * torch.cos((d - r) / ew * np.pi), 1.0)).float().contiguous()
    return halves[0], halves[1], alpha


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


def measure(a):
    import torch
    from thunder_amd import ops, postprocess, resolution
    from thunder_amd._lib import check, lib
    if not torch.cuda.is_available():
        sys.exit("postprocess_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    L = lib()
    for N in a.boxes:
        A, B, alpha = inputs(N, dev)
        n_shell, nft, n3 = N // 2 - 1, N * N * (N // 2 + 1), N ** 3
        chain = lambda **kw: postprocess.postprocess(A, B, alpha, PIXEL_SIZE, seed=SEED, **kw)
        if a.trace_run:
            for _ in range(1 + a.reps):
                chain(want_average=False)
            torch.cuda.synchronize()
            continue
        r = chain()
        rec = {"what": "postprocess", "box": N, "n_shell": n_shell, "reps": a.reps, "thres": r.thres,
               "res": r.res, "r_low": r.r_low, "n_fit": r.n_fit, "b_factor": r.b_factor,
               "status": r.status, "workspace_bytes": L.thx_postprocess_workspace(N, n_shell, 1)}
        ev = rec["events"] = {}
        ev["fsc"] = timed(lambda: resolution.masked_fsc(A, B, n_shell, mask=alpha, seed=SEED),
                          a.warmup, a.reps)
        ev["chain_estimate"] = timed(lambda: chain(want_average=False), a.warmup, a.reps)
        ev["chain_given_b"] = timed(lambda: chain(want_average=False, b_factor=GIVEN_B), a.warmup,
                                    a.reps)
        ev["chain_estimate_average"] = timed(chain, a.warmup, a.reps)
        ev["pass1_and_fit_by_difference"] = {"ms": ev["chain_estimate"]["ms"] - ev["chain_given_b"]["ms"]}
        ev["average_by_difference"] = {"ms": ev["chain_estimate_average"]["ms"]
                                       - ev["chain_estimate"]["ms"]}
        # the stage entry points alone
        F = torch.empty_like(A)
        ev["merge_weight"] = timed(lambda: check(L.thx_ft_merge_weight(
            ops._ptr(A), ops._ptr(B), N, ops._ptr(r.fsc), n_shell, ops._ptr(F), ops._stream(dev))),
            a.warmup, a.reps)
        ev["merge_weight"].update(rate(24.0 * nft, ev["merge_weight"]["ms"]))
        ev["sharpen_in_place"] = timed(lambda: postprocess.ft_sharpen(F, r.b_factor, r.res / N, 4.0 / N,
                                                                      out=F), a.warmup, a.reps)
        ev["sharpen_in_place"].update(rate(16.0 * nft, ev["sharpen_in_place"]["ms"]))
        ws = torch.empty(L.thx_bfactor_est_workspace(N, n_shell), dtype=torch.uint8, device=dev)
        out = torch.empty(4, dtype=torch.float64, device=dev)

        def est(r_dev):
            check(L.thx_bfactor_est(ops._ptr(A), N, r.r_low, n_shell, ops._ptr(r_dev), None,
                                    ops._ptr(out), None, ops._ptr(ws), ws.numel(), ops._stream(dev)))
        res_dev = torch.tensor([r.res], dtype=torch.int32, device=dev)
        one_dev = torch.tensor([1], dtype=torch.int32, device=dev)
        ev["bfactor_est_one_map"] = timed(lambda: est(res_dev), a.warmup, a.reps)
        ev["bfactor_est_one_map"].update(rate(
            8.0 * (stored_below(N, r.res) - stored_below(N, r.r_low)), ev["bfactor_est_one_map"]["ms"]))
        ev["fit_and_an_empty_pass1"] = timed(lambda: est(one_dev), a.warmup, a.reps)
        rec["bytes"] = {"k_shell_partial": 16.0 * stored_below(N, n_shell),
                        "k_guinier_partial": 16.0 * (stored_below(N, r.res) - stored_below(N, r.r_low)),
                        "k_ft_stream": 24.0 * nft, "k_pp_scale_mask": 12.0 * n3,
                        "k_random_phase": 16.0 * nft, "k_mask_mul": 12.0 * n3}
        print(json.dumps(rec), flush=True)
        with open(a.events, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del A, B, alpha, F, r, ws
        torch.cuda.empty_cache()


def kernel_stats(path):
    """{kernel: {calls, avg_ms}} from a trace directory's *kernel_stats.csv; the
    transforms' kernels are summed under "fft" per chain call"""
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_stats.csv"),
                                                           recursive=True)
    if not files:
        sys.exit(f"postprocess_bench: no kernel_stats.csv under {path}")
    out, fft_ns, calls = {}, 0.0, 0
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            hit = [k for k in KERNELS if k + "(" in name or k + "<" in name]
            if hit:
                out[hit[-1]] = {"calls": int(row["Calls"]), "avg_ms": float(row["AverageNs"]) / 1e6,
                                "min_ms": float(row["MinNs"]) / 1e6, "max_ms": float(row["MaxNs"]) / 1e6}
            elif "fft" in name.lower() or "transpose" in name.lower() or "k_col" in name:
                fft_ns += float(row["TotalDurationNs"])
    calls = out.get("k_guinier_fit", {}).get("calls", 0)
    if calls and "k_hermitian_planes" in out:
        # one kernel for both users: the FSC's four copies and the chain's own map
        out["k_hermitian_planes"]["per_chain_call"] = out["k_hermitian_planes"]["calls"] / calls
    if calls:
        out["fft_per_chain_call"] = {"calls": calls, "avg_ms": fft_ns / calls / 1e6,
                                     "note": "all transform kernels of one chain call: the FSC's four "
                                             "inverse and four forward, and the final inverse "
                                             "(the set-up runs no transform)"}
    return out


def fold(a):
    stats = dict(s.split("=", 1) for s in a.kernel_stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for line in open(a.fold):
        rec = json.loads(line)
        box = str(rec["box"])
        if box in stats:
            k = rec["kernels"] = kernel_stats(stats[box])
            for name, nbytes in rec["bytes"].items():
                if name in k:
                    k[name].update(rate(nbytes, k[name]["avg_ms"]))
        print(json.dumps(rec))
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--events", default=os.path.join(ROOT, "profiles", "postprocess_events.jsonl"))
    p.add_argument("--trace-run", action="store_true", help="only the chain, for a kernel trace")
    p.add_argument("--fold", help="an --events file to fold kernel statistics into")
    p.add_argument("--kernel-stats", nargs="*", default=[], help="BOX=trace directory or csv")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_bench.jsonl"))
    a = p.parse_args()
    if a.fold:
        fold(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
