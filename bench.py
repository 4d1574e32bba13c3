#!/usr/bin/env python3
"""Headline benchmark: particle-images/s through expectation (box 256, 2000
rotation samples), BASELINE.json metric, on N GPUs of one node.

One step = the expectation of one batch of synthetic particle images per GPU,
inputs resident in HBM: global scan over nR = 2000 rotations x nT = 151
translations at the global-search radius (rU = 24, nPxl = 870), reseed, then
10 particle-filter phases (mLR = 125, mLT = 9) -- SURVEY.md §8(d).  Weak
scaling: every rank owns its own batch (gold-standard hemisphere = rank % 2),
no collective on the expectation path.

A plain run sets up, warms up, times the steps and prints the result line
(metric, value, ms_per_step, ...); --dump-outputs DIR also writes what the
last timed step returned as DIR/<name>.npy (seeded inputs: the same arguments
give the same inputs in every run).  Everything below is measured only with
--full, beside the same headline figure.

Insert (mReco = 100), the RCCL
half-map all-reduce (thx_halfmap_allreduce over each hemisphere's ranks) and
the FSC are timed separately and reported as extra fields.

`roofline` is the dominant kernel of the timed step, k_local_fused (the
particle-filter phase at global resolution, about half the step), timed by
HIP events the driver records around every one of its launches inside the
timed region (thx_expect_cfg.phaseEvents).  The device route sends every
bench phase to the pair-form y-pair kernel k_local_fused<2>, which gathers
its taps from the driver's compact z-interleaved y-pair ball (8.7 MB at
rU 24, mostly L2-resident), so it is priced against the L2 -> L1 line
bandwidth measured by tools/probes/l2_roof.hip (random 16-B row pieces, one
128-B line each: 34.4 TB/s, the guide's L2 figure): `achieved` = SURVEY
§8(d)'s 64 B of taps per rotation-pixel per launch / launch time, and the
PMC line traffic of the same launches (tools/l2_lines.py: TCP_TCC_READ_REQ x
128 B) against the same roof says how close the kernel runs to it.  The
global scan and the full-resolution phase
are reported beside it (roofline_scan, roofline_local).

Launch: python bench.py [--gpus 1 --steps K --warmup W] [--dump-outputs DIR] [--full]
        python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from thunder_amd import expectation as ex  # noqa: E402
from thunder_amd import ops, synth  # noqa: E402
from thunder_amd._lib import lib  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3    # MI355X_MICROARCH.md, dense f32 MFMA (= VALU)
PEAK_HBM_GBS = 8000.0            # MI355X_MICROARCH.md, HBM3E spec
PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md, dense bf16 MFMA
ROOF_IMAGES = 4096               # images per global-scan launch in the roofline measurement


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--images", type=int, default=12500, help="particle images per GPU per step")
    p.add_argument("--streams", type=int, default=1,
                   help="run the --chunk sub-batches concurrently on this many HIP streams "
                        "(one host thread each)")
    p.add_argument("--chunk", type=int, default=0,
                   help="images per expectation launch (0: the whole batch in one launch; "
                        "288 GB of HBM holds the workspaces of all 12500)")
    p.add_argument("--box", type=int, default=256)
    p.add_argument("--nr", type=int, default=2000)
    p.add_argument("--phases", type=int, default=10)
    p.add_argument("--algo", type=int, default=4,
                   help="global-scan algorithm: 0 direct, 1 FP32 MFMA, 2 bf16x3 MFMA, "
                        "4 bf16x6 MFMA (exact three-way split of the FP32 operands)")
    p.add_argument("--shuffle", type=int, default=1,
                   help="1: shuffle the support before resampling (Particle::resample)")
    p.add_argument("--perturb-mean", default="acg", choices=["acg", "top"],
                   help="acg: inferACG mean of the cloud (the reference's compiled switch "
                        "PARTICLE_ROT_MEAN_USING_STAT_PERTURB); top: the top particle")
    p.add_argument("--acg-iters", type=int, default=100, help="inferACG fixed-point iteration cap")
    p.add_argument("--large-first", type=int, default=0,
                   help="1: OPTIMISER_GLOBAL_PERTURB_LARGE (off in the reference's Config.h)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step returned (rank 0's "
                        "particle clouds, weights, scores, classes and phase counts) to DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="beside the headline figure: the pose-recovery check, the rooflines (HIP "
                        "events around the phase kernel inside the timed steps, scan, "
                        "full-resolution phase, insert), the FP32-scan step, the round end "
                        "(insert, all-reduce, reconstruction, FSC) and the CPU baseline")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    p.add_argument("--cpu-images", type=int, default=4096,
                   help="images of the CPU-baseline sample (median of 3 runs)")
    p.add_argument("--no-extras", action="store_true",
                   help="with --full: skip insert / all-reduce / local roofline")
    p.add_argument("--no-rooflines", action="store_true",
                   help="with --full: keep the insert and the round end (all-reduce, reconstruction, "
                        "FSC) but skip the secondary rooflines (scan, full-resolution phase and insert)")
    a = p.parse_args()
    if a.steps < 1:
        p.error("--steps: at least one timed step")
    return a


DUMP_NAMES = ("quat", "trans", "pR", "pT", "score", "cls", "nPhase")   # Expectation.run's tuple
DUMP_BYTES = 60 * 10 ** 6


def dump_outputs(outs, path):
    """The last timed step's outputs as `path`/<name>.npy: Expectation.run's
    tuple over all sub-batches, float64 (score: float32).  Past DUMP_BYTES in all,
    a fixed seeded sample of the images (the same rows of every array, listed
    in image_index.npy)."""
    os.makedirs(path, exist_ok=True)
    arrs = [torch.cat([o[k] for o in outs]) for k in range(len(DUMP_NAMES))]
    arrs = [x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float64) for x in arrs]
    n = arrs[0].shape[0]
    per_image = sum(x[0].numel() * x.element_size() for x in arrs) + 8
    keep = min(n, DUMP_BYTES // per_image)
    idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False)) if keep < n else np.arange(n)
    sel = torch.as_tensor(idx, device=arrs[0].device)
    for name, x in zip(DUMP_NAMES, arrs):
        np.save(os.path.join(path, name + ".npy"), x[sel].cpu().numpy())
    np.save(os.path.join(path, "image_index.npy"), idx.astype(np.float64))


def rank_layout(world, rank):
    """What rank `rank` of a `world`-rank job owns (weak scaling):
    its own batch of synthetic images (seeds per rank), its gold-standard
    hemisphere (rank % 2, src/Parallel.cpp:26-53), the ranks its half-maps are
    all-reduced with, and whether it leads its hemisphere (reconstruction, and
    for A the FSC)."""
    hemi = rank % 2
    members = [r for r in range(world) if r % 2 == hemi]
    from thunder_amd.hemisphere import leads
    return {"hemisphere": hemi, "hemisphere_ranks": members, "leads": leads(world),
            "is_lead": rank in leads(world), "image_seed": 5 + 101 * rank, "pf_seed": 7 + rank}


def throughput(gpus, images, steps, seconds):
    """The bench's value: every rank's images over the max-over-ranks time."""
    return gpus * images * steps / seconds


def log(rank, *a):
    if rank == 0:
        print(*a, file=sys.stderr, flush=True)


def make_stack(N, pf, rU, rL, n_img, device, seed=5, snr=0.05, vol=None):
    """Synthetic images: ctf * shift(t_true) * P_Rtrue(vol) + noise."""
    px = ops.PixelSet(N, pf, rU, rL, device=device)
    rng = np.random.default_rng(seed)
    qtrue = torch.as_tensor(synth.uniform_quaternions(n_img, rng), device=device)
    ttrue = torch.as_tensor(rng.standard_normal((n_img, 2)) * 3.0, device=device)
    attrs = torch.as_tensor(synth.ctf_attrs(n_img, seed=seed + 1), device=device)
    ctf = ops.ctf(attrs, px)
    sig = torch.empty(n_img, px.n, dtype=torch.complex64, device=device)
    for l0 in range(0, n_img, 8192):
        l1 = min(n_img, l0 + 8192)
        P = ops.project3d(vol, ops.rotmat(qtrue[l0:l1].contiguous()), px)
        Tt = ops.trans_table(ttrue[l0:l1].contiguous(), px)
        sig[l0:l1] = ctf[l0:l1] * P * Tt
    dat, sigRcp = synth.noisy_images(sig, px.iSig, N // 2 + 1, snr=snr, seed=seed + 2)
    return px, dat, ctf, sigRcp, qtrue, ttrue


def pmc_traffic():
    """HBM bytes per launch of the roofline launch sequences, measured by the
    rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this bench (tools/gpu_round.sh
    pmc -> tools/traffic.py -> profiles/rNN_traffic.json, the newest round)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))
    if not files:
        return {}, None
    with open(files[-1]) as f:
        return json.load(f), os.path.relpath(files[-1], ROOT)


def newest_profile(pattern):
    """The newest round's profiles/<pattern> file (rNN sorts by round), or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def l2_gather_roof():
    """L2 -> L1 line bandwidth (TB/s) for random 16-B row pieces from an
    L2-resident 2 MB table: tools/probes/l2_roof.hip, profiles/rNN_l2_roof.jsonl."""
    f = newest_profile("r*_l2_roof.jsonl")
    if not f:
        return None, None
    with open(f) as fh:
        for line in fh:
            d = json.loads(line)
            if d["pattern"] == "line16" and abs(d["table_MB"] - 2.0) < 1e-6:
                return d["line_TBps"], os.path.relpath(f, ROOT)
    return None, None


def l2_lines():
    """Per-phase L1 -> L2 line requests of the bench's k_local_fused launches
    (rocprofv3 --pmc TCP_TCC_READ_REQ, tools/l2_lines.py)."""
    f = newest_profile("r*_l2_lines.json")
    if not f:
        return None, None
    with open(f) as fh:
        return json.load(fh), os.path.relpath(f, ROOT)


def timed_events(fn, reps, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record(stream)
    for _ in range(reps):
        fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) / reps / 1e3


def scan_roofline(vol, px, gset, dat, ctf, sig, algo, reps=3):
    """Average duration of the global-scan launch sequence (HIP events on the
    launch stream) priced against the matrix-core roof of its dtype:
    algo 1 = FP32 MFMA (4 flop per image x rotation x translation x pixel),
    algo 2 = bf16 MFMA, three products per FP32 product (12 bf16 flop),
    algo 4 = bf16 MFMA, six products per FP32 product (24 bf16 flop)."""
    dev = dat.device
    q, t, pR, pT = gset
    nImg, nR, nT = dat.shape[0], len(q), len(t)
    rotP = ops.project3d(vol, ops.rotmat(torch.as_tensor(q, device=dev)), px)
    traP = ops.trans_table(torch.as_tensor(t, device=dev), px)
    pRd, pTd = torch.as_tensor(pR, device=dev), torch.as_tensor(pT, device=dev)
    st = torch.cuda.current_stream(dev)
    sec = timed_events(lambda: ops.global_scan(rotP, traP, dat, ctf, sig, pRd, pTd, algo=algo),
                       reps, st)
    pad = lambda v, m: (v + m - 1) // m * m
    elems = float(pad(nImg, 64)) * pad(nR, 4) * pad(nT, 32) * pad(px.n, 16)
    issued = {2: 12.0, 4: 24.0}.get(algo, 4.0) * elems
    peak = PEAK_BF16_MFMA_TFLOPS if algo in (2, 4) else PEAK_FP32_MFMA_TFLOPS
    algorithmic = 15.0 * nImg * nR * nT * px.n      # SURVEY §8(d), direct formulation
    return sec, issued, algorithmic, peak


def local_roofline(vol, N, pf, device, n_img=512, reps=3, spreads=(1.5, 2.0, 3.0, 0.0)):
    """Full-resolution particle-filter phase (nPxl = 24746 at box 256,
    mLR = 125, mLT = 9): algorithmic bytes 64 * mLR * nPxl + 16 * nPxl per
    image-phase.  Clouds of `spreads` degrees around one pose per image (the
    narrow clouds of a C5-style local refinement; 0 = uniformly random
    rotations, every tap a gather; 2.0 = SURVEY 8(d)'s sigma), each in the half-complex layout (taps of
    compact patches staged in LDS boxes, the rest gathered row by row) and
    in the cell-expanded layout (every sample one quad-cooperative 64-B cell
    read) and the y-pair copy (pair form: two 32-B pieces per sample)."""
    rU = N // 2 - 2
    px, dat, ctf, sig, qtrue, ttrue = make_stack(N, pf, rU, 1, n_img, device, seed=17, vol=vol)
    rng = np.random.default_rng(3)
    mR, mT = 125, 9
    st = torch.cuda.current_stream(device)
    trans = torch.as_tensor(rng.standard_normal((n_img, mT, 2)), device=device)
    pC = torch.ones(n_img, dtype=torch.float64, device=device)
    pR = torch.full((n_img, mR), 1.0 / mR, dtype=torch.float64, device=device)
    pT = torch.full((n_img, mT), 1.0 / mT, dtype=torch.float64, device=device)
    cells = ops.volume_cells(vol)
    ypair = ops.volume_ypair(vol)
    out = {"clouds": []}
    for sp in spreads:
        q = (synth.clustered_quaternions(n_img, mR, sp, rng) if sp > 0
             else synth.uniform_quaternions(n_img * mR, rng).reshape(n_img, mR, 4))
        q = torch.as_tensor(np.ascontiguousarray(q), device=device)
        row = {"spread_deg": sp if sp > 0 else "uniform"}
        for name, kw in (("halfcomplex", {}), ("cells", {"cells": cells}),
                         ("ypair", {"ypair": ypair})):
            row[name + "_ms"] = timed_events(lambda: ops.local_phase(vol, q, trans, pC, pR, pT, dat,
                                                                     ctf, sig, px, **kw),
                                             reps, st) * 1e3
        out["clouds"].append(row)
    del cells, ypair
    out["algo_bytes"] = n_img * (64.0 * mR * px.n + 16.0 * px.n)
    out["nPxl"] = px.n
    out["n_img"] = n_img
    return out


def insert_fullres(vol, N, pf, device, n_img=256, m_reco=100, spread=1.5):
    """Full-resolution insert (nPxl = 24746 at box 256) of mReco samples per
    image drawn from 125-particle clouds (Particle::rand: uniform draws, so
    copies of one particle repeat); algorithmic bytes 192 mReco nPxl per image
    (8 taps x 3 floats x 8 B read-modify-write)."""
    rU = N // 2 - 2
    px, dat, ctf, sig, qtrue, ttrue = make_stack(N, pf, rU, 1, n_img, device, seed=19, vol=vol)
    rng = np.random.default_rng(4)
    q = torch.as_tensor(np.ascontiguousarray(synth.clustered_quaternions(n_img, 125, spread, rng)),
                        device=device)
    t = torch.as_tensor(rng.standard_normal((n_img, 9, 2)), device=device)
    iq, it = ex.draw_insert_samples(q, t, m_reco)
    off = torch.zeros(n_img, 2, dtype=torch.float64, device=device)
    w = torch.full((n_img,), 1.0 / m_reco, dtype=torch.float32, device=device)
    hm = ops.HalfMap(N * pf, device)
    st = torch.cuda.current_stream(device)
    sec = timed_events(lambda: ops.insert3d(hm, dat, ctf, iq, it, off, w, px), 2, st)
    algo = 192.0 * m_reco * px.n * n_img
    return {"images": n_img, "mReco": m_reco, "nPxl": px.n, "ms": sec * 1e3,
            "images_per_s": n_img / sec, "algorithmic_bytes": algo,
            "algorithmic_TBps": algo / sec / 1e12, "method": ops.insert_method(hm, m_reco, px),
            "note": "clouds of 125 particles at %.1f deg, mReco uniform draws" % spread}


def cpu_info():
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, os.cpu_count()


def cpu_share():
    """The host CPUs this process may use: the affinity mask, the cgroup CPU
    quota (cgroup v2 cpu.max or v1 cfs_quota/period) and OMP_NUM_THREADS (the
    per-GPU share the box exports).  Threads = the smallest of them."""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = int(q) / int(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    omp = os.environ.get("OMP_NUM_THREADS")
    omp = int(omp) if omp and omp.isdigit() else None
    threads = aff
    if quota:
        threads = min(threads, max(1, int(math.floor(quota))))
    if omp:
        threads = min(threads, omp)
    return {"threads": threads, "affinity_cpus": aff, "cgroup_quota_cpus": quota,
            "omp_num_threads": omp, "nproc": os.cpu_count()}


def cpu_baseline(vol_np, N, pf, gset, dat, ctf, sig, px, phases, n_img=4096, runs=3):
    """The CPU path (oracle/cpu_fast.c: the reference's expectation loop
    structure, OpenMP, -O3 -march=native, likelihood vectorised over images in
    the scan and over pixels in the phases) on the host cores this process
    may use (cpu_share), same workload shape per image: the median of `runs`
    runs over the same n_img-image sample."""
    import ctypes
    from oracle import oracle as orc
    orc.build()
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libcpufast.so"))
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    share = cpu_share()
    threads = share["threads"]
    os.environ["OMP_NUM_THREADS"] = str(threads)
    L.cpu_set_threads(threads)
    q, t, pR, pT = (np.ascontiguousarray(x) for x in gset)
    vdim = pf * N
    mR, mT = 125, 9
    rng = np.random.default_rng(0)
    vol_np = np.ascontiguousarray(vol_np)
    iCol, iRow = np.ascontiguousarray(px.iCol), np.ascontiguousarray(px.iRow)
    n = min(n_img, len(dat))
    lq = np.ascontiguousarray(synth.clustered_quaternions(n * phases, mR, 3.0, rng))
    lt = np.ascontiguousarray(rng.standard_normal((n * phases, mT, 2)))
    d, c, s_ = (np.ascontiguousarray(x[:n]) for x in (dat, ctf, sig))

    def run():
        base = np.zeros(n, np.float32)
        lb = np.zeros(n, np.float32)
        t0 = time.perf_counter()
        L.cpu_step(P(vol_np), vdim, pf, P(q), len(q), P(t), len(t), P(pR), P(pT), P(d), P(c), P(s_),
                   n, P(iCol), P(iRow), px.n, N, P(lq), mR, P(lt), mT, phases, P(base), P(lb))
        return time.perf_counter() - t0

    dts = sorted(run() for _ in range(runs))
    dt = dts[len(dts) // 2]
    model, ncpu = cpu_info()
    return {"value": n / dt, "unit": "particle-images/s", "cores": threads, "kind": "port",
            "cpu_model": model, "nproc": ncpu, "build": "gcc -O3 -march=native -fopenmp",
            "cpu_share": share, "runs_s": [round(x, 2) for x in dts],
            "spread": (dts[-1] - dts[0]) / dt,
            "sample": f"{n} images x (global scan nR={len(q)} nT={len(t)} nPxl={px.n} + "
                      f"{phases} local phases {mR}x{mT}), oracle/cpu_fast.c, OpenMP {threads} "
                      f"threads, median of {runs} runs ({dt:.1f} s)",
            "note": "the builder's CPU port of the reference's loop structure (FP32, OpenMP, "
                    "vectorised over images / pixels); its speed relative to the reference's "
                    "own logDataVSPrior_m_n_huabin_SIMD256 loop (src/Optimiser.cpp:9931-9973) "
                    "is not calibrated: the reference's CPU path cannot be built here (Boost)"}


PEAK_FP32_TFLOPS = PEAK_FP32_MFMA_TFLOPS


def main():
    a = parse()
    # gloo and RCCL print banners on the process's C stdout; the contract is ONE
    # JSON line there, so fd 1 points at stderr until rank 0 prints the line
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    # (local % device count: lets a one-GPU box rehearse the multi-rank path
    # with THX_BENCH_BACKEND=gloo; on a node local < device count)
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    backend = os.environ.get("THX_BENCH_BACKEND", "nccl")
    cdev = dev if backend == "nccl" else torch.device("cpu")   # collectives' tensors
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    lib()   # fail loudly if the HIP library is missing

    N, pf, rU, rL = a.box, 2, 24, 1
    mR, mT = 125, 9
    log(rank, f"[bench] building synthetic volume N={N} pf={pf}")
    vol = synth.projectee(synth.blob_volume(N, seed=1, device=dev), pf)
    # a3 on device (Particle::reset through thx_global_sample_set); sizes by the
    # reference's rules (thx_global_sample_sizes: nT = 151 at transS 10)
    _, nR, nT = ops.global_sample_sizes(a.nr)
    gset = tuple(x.cpu().numpy() for x in ops.global_sample_set(nR, nT, 10.0, 2, dev))
    lay = rank_layout(world, rank)
    px, dat, ctf, sig, qtrue, ttrue = make_stack(N, pf, rU, rL, a.images, dev, seed=lay["image_seed"],
                                                 vol=vol)
    mk = lambda algo: ex.Expectation(vol, px, gset, n_phase=a.phases, algo=algo, seed=lay["pf_seed"],
                                     shuffle=bool(a.shuffle), perturb_mean=a.perturb_mean,
                                     acg_iters=a.acg_iters, large_first=bool(a.large_first))
    e = mk(a.algo)
    chunk = a.chunk or a.images
    chunks = [(l0, min(a.images, l0 + chunk)) for l0 in range(0, a.images, chunk)]
    outs = [None] * len(chunks)
    # --full: HIP events around every k_local_fused launch of the timed steps (one
    # launch per phase when the batch runs as one expectation call)
    timer = (ex.PhaseTimer(e, a.phases * a.steps)
             if a.full and len(chunks) == 1 and a.phases else None)

    streams = [torch.cuda.Stream(dev) for _ in range(a.streams)] if a.streams > 1 else None

    def run_chunks(cs, stream=None):
        for c in cs:
            l0, l1 = chunks[c]
            if stream is None:
                outs[c] = e.run(dat[l0:l1], ctf[l0:l1], sig[l0:l1], out=outs[c])
            else:
                with torch.cuda.stream(stream):
                    outs[c] = e.run(dat[l0:l1], ctf[l0:l1], sig[l0:l1], out=outs[c])

    def step(i=None):
        if timer is not None and i is not None:
            timer.select(i * a.phases)
        if streams is None:
            run_chunks(range(len(chunks)))
            return
        # sub-batches round-robin over the streams, one host thread per stream
        # (the driver's calls release the GIL); the streams join the default one
        import threading
        cur = torch.cuda.current_stream(dev)
        for st in streams:
            st.wait_stream(cur)
        th = [threading.Thread(target=run_chunks, args=(range(k, len(chunks), len(streams)), st))
              for k, st in enumerate(streams)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for st in streams:
            cur.wait_stream(st)

    log(rank, f"[bench] nPxl={px.n} nR={a.nr} nT={len(gset[1])} images/gpu={a.images}")
    if timer is not None:
        e.cfg.phaseEvents = None
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if dist:
        tt = torch.tensor([el], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
    ms_per_step = el / a.steps * 1e3
    value = throughput(a.gpus, a.images, a.steps, el)
    local_ms = timer.ms() if timer is not None else []
    if timer is not None:
        timer.close()
    if a.dump_outputs and rank == 0:
        dump_outputs(outs, a.dump_outputs)

    # accuracy sanity of the timed path: top rotation vs true pose
    res = {}
    if a.full and rank == 0:
        # (off-grid poses: a 2000-rotation grid at the 15 A scan resolution
        # leaves about half the modes in a wrong basin; tools/diag_expect.py)
        qa = outs[0][0]
        q0 = ex.cloud_mode(qa)
        qt = qtrue[:q0.shape[0]]
        cosang = (q0 * qt).sum(-1).abs().clamp(max=1)
        res["median_pose_error_deg"] = float(torch.rad2deg(2 * torch.acos(cosang)).median())
        # final particle-cloud spread: angle of every rotation sample to the cloud mode
        ca = (qa * q0[:, None, :]).sum(-1).abs().clamp(max=1)
        ang = torch.rad2deg(2 * torch.acos(ca))
        qs = torch.tensor([0.1, 0.5, 0.9], dtype=ang.dtype, device=ang.device)
        res["cloud_spread_deg"] = {
            "median_p10_p50_p90": [round(float(v), 2) for v in torch.quantile(ang.median(1).values, qs)],
            "max_p10_p50_p90": [round(float(v), 2) for v in torch.quantile(ang.max(1).values, qs)]}

    extras = {}
    traffic, traffic_src = pmc_traffic() if a.full else ({}, None)

    def launch_traffic(key, ok):
        t = traffic.get(key) if ok else None
        return (t["traffic_bytes"], f"{traffic_src}: {key}") if t else (None, None)

    # ---- dominant kernel of the timed step: k_local_fused (routed per phase)
    if local_ms:
        nL = chunks[0][1] - chunks[0][0]
        per_img = 56.0 * mR * px.n + 15.0 * mR * mT * px.n        # SURVEY §8(d), per image-phase
        flop = nL * per_img
        t_launch = float(np.mean(local_ms)) / 1e3
        achieved = flop / t_launch / 1e12
        tr, tr_src = launch_traffic("local_bench", N == 256 and a.nr == 2000 and nL == 12500)
        tap_bytes = 64.0 * mR * px.n * nL
        roof, roof_src = l2_gather_roof()
        roof = roof or 34.5           # MI355X_MICROARCH.md, L2 per XCD x 8
        by_phase = ([float(np.mean(local_ms[k::a.phases])) for k in range(a.phases)]
                    if len(local_ms) == a.phases * a.steps else None)
        lines, lines_src = l2_lines() if (N == 256 and a.nr == 2000 and nL == 12500) else (None, None)
        line_fields = {}
        if lines and by_phase and len(lines["per_phase"]) == a.phases:
            lb = [p["TCP_TCC_READ_REQ_sum"] * 128.0 for p in lines["per_phase"]]
            rate = [b / (ms / 1e3) / 1e12 for b, ms in zip(lb, by_phase)]
            line_fields = {
                "l2_line_bytes_per_launch": float(np.mean(lb)),
                "l2_line_TBps_by_phase": [round(r, 2) for r in rate],
                "l2_line_frac_by_phase": [round(r / roof, 3) for r in rate],
                "l2_line_frac": float(np.sum(lb) / (np.sum(by_phase) / 1e3) / 1e12 / roof),
                "l2_lines_per_sample_by_phase": [round(p["TCP_TCC_READ_REQ_sum"] / (mR * px.n * nL), 2)
                                                 for p in lines["per_phase"]],
                "l2_hit_rate": float(lines["mean"]["TCC_HIT_sum"] /
                                     (lines["mean"]["TCC_HIT_sum"] + lines["mean"]["TCC_MISS_sum"])),
                "l2_lines_source": lines_src}
        extras["roofline"] = {
            "bound": "l2", "achieved": tap_bytes / t_launch / 1e12, "peak": roof, "unit": "TB/s",
            "frac": tap_bytes / t_launch / 1e12 / roof, "traffic": tr,
            "traffic_unit": "bytes per launch (HBM, PMC)", "traffic_source": tr_src,
            "peak_source": roof_src or "MI355X_MICROARCH.md L2", **line_fields,
            "kernel": f"k_local_fused (particle-filter phase, nPxl={px.n}, {mR}x{mT}, {nL} images "
                      "per launch), routed on the device per phase: the staged half-complex kernel "
                      "<0> where the LDS boxes pay, else the pair-form y-pair kernel <2> on the "
                      "driver's compact z-interleaved y-pair ball",
            "launch_ms": t_launch * 1e3, "launches_timed": len(local_ms),
            "launch_ms_by_phase": [round(float(np.mean(local_ms[k::a.phases])), 3)
                                   for k in range(a.phases)] if len(local_ms) == a.phases * a.steps else None,
            "share_of_step": float(np.sum(local_ms)) / (a.steps * ms_per_step),
            "algorithmic_flop_per_launch": flop,
            "fp32_TFLOPs": achieved, "fp32_frac": achieved / PEAK_FP32_TFLOPS,
            "tap_bytes_per_launch": tap_bytes,
            "note": "HIP events recorded by the driver on its launch stream around every "
                    "phase's routed k_local_fused launches of the timed steps (two dispatches, "
                    "one exits at entry; rocprof lists them per variant); achieved = 64 B of taps per "
                    "rotation-pixel (SURVEY 8(d)) per launch / launch time, peak = the L2 -> L1 "
                    "line bandwidth for random 16-B row pieces (tools/probes/l2_roof.hip, = the "
                    "guide's L2 figure); each tap row piece costs a 128-B line unless L1 or the "
                    "LDS patch box serves it, so the line traffic (PMC, l2_line_*) runs at the roof "
                    "while the algorithmic rate is a fraction of it"}

    if a.full and not a.no_extras and not a.no_rooflines:
        # ---- secondary: the global scan (bf16x6 MFMA) and its FP32-MFMA twin
        nRoof = min(ROOF_IMAGES, a.images)
        sec, issued, algorithmic, peak = scan_roofline(vol, px, gset, dat[:nRoof], ctf[:nRoof],
                                                       sig[:nRoof], a.algo)
        kname = {1: "k_scan_mfma (fp32 32x32x2)", 2: "k_scan_split<BF16X3> (bf16 32x32x16, 3-product split)",
                 4: "k_scan_split<BF16X6> (bf16 32x32x16, exact 3-way split, 6 products)"}
        tr, tr_src = launch_traffic("scan_4096", a.algo == 4 and nRoof == 4096
                                    and a.nr == 2000 and N == 256)
        extras["roofline_scan"] = {
            "bound": "mfma", "achieved": issued / sec / 1e12, "peak": peak, "unit": "TFLOP/s",
            "frac": issued / sec / 1e12 / peak, "traffic": tr,
            "traffic_unit": "bytes per launch (HBM, PMC)", "traffic_source": tr_src,
            "kernel": f"global scan {kname.get(a.algo, a.algo)} + prep + combine",
            "launch_ms": sec * 1e3, "images_per_launch": nRoof,
            "algorithmic_equiv_tflops": algorithmic / sec / 1e12,
            "note": "achieved = issued matrix-core flops after the expansion of |d-cTP|^2 into a "
                    "GEMM (4 fp32 flop, or 6x4 bf16 flop for bf16x6, per image x rotation x "
                    "translation x pixel); algorithmic_equiv uses the direct 15-flop count of "
                    "SURVEY 8(d)"}
        sec1, issued1, _, _ = scan_roofline(vol, px, gset, dat[:nRoof], ctf[:nRoof], sig[:nRoof], 1)
        extras["roofline_scan"]["fp32_mfma_launch_ms"] = sec1 * 1e3
        extras["roofline_scan"]["fp32_mfma_frac"] = issued1 / sec1 / 1e12 / PEAK_FP32_MFMA_TFLOPS
        if a.algo != 1:
            # whole-step throughput with the FP32-MFMA scan (algo 1) beside the headline
            e1 = mk(1)
            o1 = e1.run(dat, ctf, sig)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(2):
                e1.run(dat, ctf, sig, out=o1)
            torch.cuda.synchronize()
            extras["images_per_s_fp32_scan"] = a.gpus * a.images * 2 / (time.perf_counter() - t1)
            del e1, o1

        # ---- secondary: the north-star full-resolution phase against HBM
        lr = local_roofline(vol, N, pf, dev)
        lbytes = lr["algo_bytes"]
        frac = lambda ms: lbytes / (ms / 1e3) / 1e9 / PEAK_HBM_GBS
        # the PMC bytes of the same dispatches (tools/traffic.py: per cloud and
        # layout, exact 64 / 128-B split where the pmc3 pass has it)
        lt = traffic.get("local_fullres_512") if N == 256 else None
        clouds = []
        lays = ("halfcomplex", "cells", "ypair")
        for row in lr["clouds"]:
            best = min(lays, key=lambda k: row[k + "_ms"])
            c = {**{k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()},
                 **{"algorithmic_frac_" + k: round(frac(row[k + "_ms"]), 3) for k in lays},
                 "best": best}
            key = "uniform" if row["spread_deg"] == "uniform" else f"{float(row['spread_deg']):.1f}"
            pm = (lt or {}).get(key, {})
            for k in lays:
                if k in pm:
                    tb = pm[k]["traffic_bytes"] / (row[k + "_ms"] / 1e3) / 1e12
                    c["hbm_TBps_" + k] = round(tb, 3)
                    c["hbm_frac_" + k] = round(tb * 1e3 / PEAK_HBM_GBS, 3)
                    c["hbm_bytes_exact_" + k] = "exact_read" in pm[k]
            clouds.append(c)
        head = clouds[0]
        best = head["best"]
        lsec = head[best + "_ms"] / 1e3
        hk = "uniform" if head["spread_deg"] == "uniform" else f"{float(head['spread_deg']):.1f}"
        pm = ((lt or {}).get(hk) or {}).get(best)
        tr = pm["traffic_bytes"] if pm else None
        hbm = tr / lsec / 1e9 if tr else None
        extras["roofline_local"] = {
            "bound": "hbm", "achieved": hbm, "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": hbm / PEAK_HBM_GBS if hbm else None, "traffic": tr,
            "traffic_unit": "bytes per launch (HBM / fabric reads + writes, PMC, of the same "
                            "kernel, cloud and layout as the time)",
            "traffic_source": f"{traffic_src}: local_fullres_512/{hk}/{best}" if tr else None,
            "algorithmic_bytes": lbytes,
            "algorithmic_GBps": lbytes / lsec / 1e9,
            "algorithmic_frac": lbytes / lsec / 1e9 / PEAK_HBM_GBS,
            "kernel": f"local phase full-res (nPxl={lr['nPxl']}, 125x9, {lr['n_img']} images), "
                      f"{head['spread_deg']} deg local-search clouds, the faster projectee layout "
                      f"({best}); every cloud and layout in by_cloud",
            "note": "achieved / frac = PMC bytes moved between L2 and the fabric (HBM, MALL "
                    "hits included) per launch / launch time; algorithmic_* = 64 B of taps per "
                    "rotation-pixel + 16 B per pixel (SURVEY 8(d)) / launch time, which L2 / MALL "
                    "reuse of the narrow clouds can lift past what HBM delivers",
            "launch_ms": lsec * 1e3, "by_cloud": clouds}
        extras["insert_fullres"] = insert_fullres(vol, N, pf, dev)

    if a.full and not a.no_extras:
        # ---- insert (mReco = 100) into the two hemispheres' half-maps, the
        # per-hemisphere RCCL all-reduce, FSC between the half-maps
        quat, trans = outs[0][0], outs[0][1]
        iq, it = ex.draw_insert_samples(quat, trans, 100)
        nI = iq.shape[0]
        offS = torch.zeros(nI, 2, dtype=torch.float64, device=dev)
        w = torch.full((nI,), 1.0 / 100, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev)
        if world == 1:
            # one GPU holds both hemispheres: odd / even images
            recs = [ex.Reconstructor(N, pf, dev) for _ in range(2)]
            halves = [torch.arange(h, nI, 2, device=dev) for h in (0, 1)]
            parts = [(dat[hh].contiguous(), ctf[hh].contiguous(), iq[hh].contiguous(),
                      it[hh].contiguous(), offS[hh].contiguous(), w[hh].contiguous()) for hh in halves]

            def ins():
                for r_, p_ in zip(recs, parts):
                    r_.insert(*p_, px)
        else:
            recs = [ex.Reconstructor(N, pf, dev)]

            def ins():
                recs[0].insert(dat[:nI], ctf[:nI], iq, it, offS, w, px)
        isec = timed_events(ins, 2, st)
        extras["insert_images_per_s"] = a.gpus * nI / isec
        hm_bytes = recs[0].hm.F.numel() * 8 + recs[0].hm.T.numel() * 4
        if dist:
            # the round end across ranks (thunder_amd.hemisphere): RCCL sum of
            # each hemisphere's half-maps, reconstruction on the hemisphere
            # leads, B's map handed to A's lead (xGMI peer transfer), FSC there
            from thunder_amd import hemisphere as hs
            re_ = hs.RoundEnd(world, rank, transport="rccl" if backend == "nccl" else "torch",
                              device=cdev)
            torch.cuda.synchronize()
            dist.barrier()
            t1 = time.perf_counter()
            re_.reduce(recs[0].hm)
            torch.cuda.synchronize()
            extras["allreduce_ms"] = (time.perf_counter() - t1) * 1e3
            extras["allreduce_bytes"] = hm_bytes
            extras["allreduce_ranks_per_hemisphere"] = len(lay["hemisphere_ranks"])
            extras["allreduce_transport"] = re_.transport
            if re_.is_lead:
                ops.reconstruct(recs[0].hm, N, pf, want_ft=False)   # hipFFT plans (first call)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                mine = ops.reconstruct(recs[0].hm, N, pf)[1]
                torch.cuda.synchronize()
                extras["reconstruct_ms_per_halfmap"] = (time.perf_counter() - t1) * 1e3
                t1 = time.perf_counter()
                got = re_.exchange(mine)
                torch.cuda.synchronize()
                extras["exchange_ms"] = (time.perf_counter() - t1) * 1e3
                extras["exchange_bytes"] = mine.numel() * 8
                if got is not None:
                    fsc = ops.fsc(got[0], got[1], N // 2)
                    extras["reconstructed_fsc_shells_4_16_32_64"] = [
                        round(float(fsc[k]), 4) for k in (4, 16, 32, 64) if k < fsc.numel()]
            dist.barrier()
            re_.close()
        else:
            extras["allreduce_ms"] = 0.0
            extras["allreduce_note"] = "1 GPU: both hemispheres on one device, no all-reduce"
            fsc = ops.fsc(recs[0].hm.F, recs[1].hm.F, N)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fsc = ops.fsc(recs[0].hm.F, recs[1].hm.F, N)
            torch.cuda.synchronize()
            extras["fsc_ms"] = (time.perf_counter() - t1) * 1e3
            # f1: reconstruct both half-maps (grid-corrected solve, hipFFT at
            # box pf N), FSC of the reconstructed maps
            # (a first call makes the hipFFT plans -- kernels compiled at run
            # time on a fresh box -- which stay cached for later iterations)
            # the two hemispheres' solves: one after the other on one stream
            # (each solve is HBM-bound: r04q measured two streams from two host
            # threads at 2.7x one solve, worse than serial), and, for the
            # record, on two streams from two host threads (per-stream hipFFT
            # plans and workspaces)
            import threading
            streams = [torch.cuda.Stream(dev) for _ in recs]
            recs_out = [None] * len(recs)
            T0 = [r_.hm.T.clone() for r_ in recs]

            def reset_T():
                for r_, t0 in zip(recs, T0):
                    r_.hm.T.copy_(t0)                 # thx_reconstruct modifies T in place
                torch.cuda.synchronize()

            def solve(k):
                with torch.cuda.stream(streams[k]):
                    recs_out[k] = ops.reconstruct(recs[k].hm, N, pf)
                streams[k].synchronize()

            def both_concurrent():
                th = [threading.Thread(target=solve, args=(k,)) for k in range(len(recs))]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                torch.cuda.synchronize()

            def both_serial():
                for k in range(len(recs)):
                    recs_out[k] = ops.reconstruct(recs[k].hm, N, pf)
                torch.cuda.synchronize()

            both_concurrent()                         # plans per stream (first call)
            reset_T()
            both_serial()                             # this stream's plans
            reset_T()
            t1 = time.perf_counter()
            both_concurrent()
            extras["reconstruct_ms_two_halfmaps_concurrent"] = (time.perf_counter() - t1) * 1e3
            reset_T()
            t1 = time.perf_counter()
            both_serial()
            extras["reconstruct_ms_two_halfmaps"] = (time.perf_counter() - t1) * 1e3
            extras["reconstruct_ms_per_halfmap"] = extras["reconstruct_ms_two_halfmaps"] / 2
            extras["reconstruct_balancing_iterations"] = [o[2] for o in recs_out]
            # one half-map's solve alone, for the concurrency ratio
            hm1 = ops.HalfMap(recs[0].hm.vdim, dev)
            hm1.F.copy_(recs[0].hm.F)
            hm1.T.copy_(T0[0])
            ops.reconstruct(hm1, N, pf)               # this stream's plans (first call)
            hm1.T.copy_(T0[0])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ops.reconstruct(hm1, N, pf)
            torch.cuda.synchronize()
            extras["reconstruct_ms_one_halfmap_alone"] = (time.perf_counter() - t1) * 1e3
            del hm1
            fsc = ops.fsc(recs_out[0][1], recs_out[1][1], N // 2)
            extras["reconstructed_fsc_shells_4_16_32_64"] = [round(float(fsc[k]), 4)
                                                           for k in (4, 16, 32, 64)]

    if a.full and rank == 0 and not a.no_cpu_baseline:
        vol_np = vol.cpu().numpy()
        n_cpu = min(a.cpu_images, dat.shape[0])
        extras["cpu_baseline"] = cpu_baseline(vol_np, N, pf, gset, dat[:n_cpu].cpu().numpy(),
                                              ctf[:n_cpu].cpu().numpy(), sig[:n_cpu].cpu().numpy(),
                                              px, a.phases, n_img=n_cpu)

    if rank == 0:
        line = {"metric": "particle-images/sec through expectation (box 256, 2000 rot samples)",
                "value": value, "unit": "particle-images/s", "n_gpus": a.gpus, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None,
                "dtype": {1: "f32", 4: "f32 (global scan: FP32 operands split exactly into three bf16, "
                               "six products -- dropped terms <= 2^-24 |w||T| each, comparable to an FP32 product's "
                               "rounding -- FP32 accumulation, cancellation-guarded direct FP32 "
                               "recompute; phases: FP32)"}.get(
                    a.algo, "f32 with a bf16x3 global scan (narrower than FP32)"),
                "data": "synthetic (seeded Gaussian-blob volume, CTF-modulated noisy projections, SNR 0.05)",
                "config": {"workload": f"C3: 3D refine box {N}, {a.nr} rotation x {len(gset[1])} "
                                       f"translation global scan at rU={rU} (nPxl={px.n}) + "
                                       f"{a.phases} particle-filter phases ({mR} x {mT})",
                           "images_per_gpu": a.images, "global_batch": a.images * a.gpus,
                           "box": N, "pf": pf, "nR": a.nr, "nT": len(gset[1]), "nPxl": px.n,
                           "scan_algo": a.algo, "perturb_mean": a.perturb_mean,
                           "parallelism": f"dp{a.gpus} (hemisphere = rank % 2)"},
                **res, **extras}
        sys.stdout.flush()
        os.dup2(json_fd, 1)
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
