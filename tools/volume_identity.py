#!/usr/bin/env python3
"""Bit identity of the map-level entry points across two builds of the library
(csrc/volume.h's shared pieces, thx::bind_plans, the moved macros) and of the
particle statistics' (the thx_pf_* rows, --only thx_pf_ for those): every row
runs twice in this process with the library THX_LIB names, on fixed inputs, and
the first run's output tensors go to an .npz; --compare puts two such files
side by side, one JSON line per row.

    THX_LIB=thunder_amd/ab/lib_parent.so python tools/volume_identity.py --dump parent.npz
    python tools/volume_identity.py --dump child.npz
    python tools/volume_identity.py --compare parent.npz child.npz \\
        --out profiles/volume_helpers_identity.jsonl

A measurement driver, not a test: every row is documented as deterministic, so
a row that differs between the libraries is a defect of the child, and a row
that is not run-to-run identical on the parent is reported and left out of the
verdict.  --compare needs no GPU.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 11
BIG = 16 << 20      # bytes above which the .npz keeps a tensor's digest


def halves(N, seed=3):
    """two noisy copies of one smooth field under exp(-20 (u/N)^2), and a soft sphere"""
    rng = np.random.default_rng(seed + N)
    ax = np.fft.fftfreq(N, 1.0 / N)
    u2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + np.abs(ax[None, None, :N // 2 + 1]) ** 2
    shape = u2.shape
    field = lambda: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    signal = field() * np.exp(-20.0 * u2 / (N * N))
    sigma = np.sqrt(6.0) * np.exp(-20.0 / 9.0)
    A, B = ((signal + sigma * field()).astype(np.complex64) for _ in range(2))
    d = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    r, ew = 0.3 * N, 4.0
    alpha = np.where(d > r + ew, 0.0, np.where(d >= r, 0.5 + 0.5 * np.cos((d - r) / ew * np.pi), 1.0))
    return A, B, alpha.astype(np.float32)


def rows():
    """(name, thunk) pairs; a thunk returns {tensor name: numpy array}"""
    import torch
    from thunder_amd import ops, postprocess, reference, resolution, subtract, synth
    from thunder_amd._lib import check, lib
    from thunder_amd.ops import _ptr
    dev = torch.device("cuda", 0)
    L = lib()
    T_ = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)

    def host(v):
        if v is None:
            return np.zeros(0)
        return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

    def fields(r):
        return {k: host(getattr(r, k)) for k in r._fields}

    out = []
    cache = {}

    def hv(N):
        if N not in cache:
            cache.clear()
            cache[N] = halves(N)
        return cache[N]

    for N, method in ((32, 1), (32, 2), (48, 1), (144, 1)):
        for branch in ("alpha", "core"):
            def fsc(N=N, method=method, branch=branch):
                A, B, alpha = hv(N)
                kw = dict(mask=T_(alpha)) if branch == "alpha" else dict(core_radius=0.3 * N)
                return fields(resolution.masked_fsc(T_(A), T_(B), N // 2 - 1, edge=4.0, seed=SEED,
                                                    method=method, **kw))
            out.append((f"thx_fsc_masked N={N} method={method} {branch}", fsc))

    for N in (32, 48, 144):
        for b in (None, -50.0):
            for avg in (True, False):
                def pp(N=N, b=b, avg=avg):
                    A, B, alpha = hv(N)
                    return fields(postprocess.postprocess(T_(A), T_(B), T_(alpha), 1.0, seed=SEED,
                                                          b_factor=b, method=1, want_average=avg))
                out.append((f"thx_postprocess N={N} b={'estimated' if b is None else 'given'} "
                            f"average={int(avg)}", pp))

    for N, rL, rU in ((16, 1, 7), (144, 1, 72)):
        for use_dev in (False, True):
            def est(N=N, rL=rL, rU=rU, use_dev=use_dev):
                rng = np.random.default_rng(8)
                ax = np.fft.fftfreq(N, 1.0 / N)
                u = np.rint(np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2
                                    + ax[None, None, :N // 2 + 1] ** 2))
                F = T_((np.exp(2.0 - 30.0 * (u / N) ** 2) * (1 + 0.2 * rng.random(u.shape))
                        * np.exp(2j * np.pi * rng.random(u.shape))).astype(np.complex64))
                w = T_(0.5 + rng.random(N // 2))
                cap = N // 2 if use_dev else rU
                r_dev = torch.tensor([rU], dtype=torch.int32, device=dev) if use_dev else None
                ws = torch.empty(L.thx_bfactor_est_workspace(N, N // 2), dtype=torch.uint8, device=dev)
                res = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
                g = torch.full((2, cap), -7.0, dtype=torch.float64, device=dev)
                check(L.thx_bfactor_est(_ptr(F), N, rL, cap, _ptr(r_dev), _ptr(w), _ptr(res), _ptr(g),
                                        _ptr(ws), ws.numel(), None))
                return {"out": host(res), "guinier": host(g)}
            out.append((f"thx_bfactor_est N={N} rU={'device' if use_dev else 'host'}", est))

    for N, pf in ((16, 2), (22, 2), (16, 3), (32, 1), (200, 2), (64, 2), (32, 4), (128, 2), (64, 1)):
        for method in (1, 2):
            def rec(N=N, pf=pf, method=method):
                vdim = N * pf
                g = torch.Generator(device=dev).manual_seed(vdim + pf)
                ax = torch.fft.fftfreq(vdim, 1.0 / vdim, device=dev)
                quad = ax.view(-1, 1, 1) ** 2 + ax.view(1, -1, 1) ** 2 + ax[:vdim // 2 + 1].abs().view(1, 1, -1) ** 2
                quad[:, :, vdim // 2] = ax.view(-1, 1) ** 2 + ax.view(1, -1) ** 2 + (vdim / 2) ** 2
                T = (50.0 / (1.0 + quad.sqrt()) * (0.8 + 0.4 * torch.rand(quad.shape, generator=g, device=dev))
                     ).float().contiguous()
                try:
                    W, it, diffs = ops.reconstruct_weights(T, N, pf, method=method)
                except Exception as e:      # a method the box does not serve: the same refusal on both
                    return {"error": np.frombuffer(type(e).__name__.encode(), np.uint8)}
                return {"W": host(W), "nIter": np.array(it), "diffs": np.array(diffs, np.float64),
                        "T_after": host(T)}
            out.append((f"thx_reconstruct_weights N={N} pf={pf} method={method}", rec))

    def volume(N):
        return np.random.default_rng(100 + N).standard_normal((N, N, N)).astype(np.float32)

    for N, pf, method in ((16, 2, "pruned"), (32, 2, "pruned"), (64, 1, "pruned"), (24, 2, "fallback"),
                          (32, 2, "fallback")):
        for from_ft in (False, True):
            def prj(N=N, pf=pf, method=method, from_ft=from_ft):
                src = T_(volume(N))
                if from_ft:
                    src = torch.fft.rfftn(src).to(torch.complex64).contiguous()
                return {"projectee": host(reference.refresh_projectee(src, pf, N / 4, None, edge=6,
                                                                      method=method))}
            out.append((f"thx_projectee N={N} pf={pf} {method} fromFT={int(from_ft)}", prj))

    for N in (16, 32):
        def cen(N=N):
            co = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(np.float64)
            k, j, i = np.meshgrid(co, co, co, indexing="ij")
            d = np.sqrt((i - N / 8) ** 2 + (j + 1.5 * N / 16) ** 2 + (k - 3.0 * N / 16) ** 2)
            m = np.exp(-np.maximum(d - N / 8, 0) ** 2 / (2 * (N / 12) ** 2)).astype(np.float32)
            return {"centroid": host(subtract.region_centroid(T_(m)))}
        out.append((f"thx_region_centroid N={N}", cen))

    for N, r in ((32, 15), (64, 31), (32, 10)):
        def sub(N=N, r=r):
            n, pf = 7, 2
            rng = np.random.default_rng(3 + N + r)
            vols = np.stack([synth.projectee(synth.blob_volume(N, n_blobs=30, seed=s), pf).numpy()
                             for s in (1, 2)])
            ori = (rng.standard_normal((n, N, N // 2 + 1)) + 1j * rng.standard_normal((n, N, N // 2 + 1))
                   ).astype(np.complex64)
            cls = np.array([0, 1, 1, 0, 1, 0, 0], np.int32)
            dF = np.array([1.0, 1.02, 1.0, 0.97, 1.0, 1.0, 1.01])
            o = subtract.subtract(T_(vols), T_(ori), T_(synth.ctf_attrs(n, seed=8)),
                                  T_(synth.uniform_quaternions(n, rng)), T_(rng.standard_normal((n, 2)) * 2),
                                  r, pf, T_(rng.standard_normal((n, 2)) * 1.5), T_(dF), T_(cls),
                                  ops.symmetry("D2")[0], T_(np.array([1.5, -2.25, 0.75]) * (N / 32)),
                                  real=True, model=True)
            return {k: host(v) for k, v in vars(o).items() if torch.is_tensor(v)}
        out.append((f"thx_subtract N={N} r={r} D2 diffRL", sub))

    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def expose_wt():
        from oracle import reconstruct as orc_rc
        N, pf, tab_n = 32, 2, 100000
        vdim, maxR = N * pf, N // 2 - 2
        tab = orc_rc.mkb_rl_r2(np.arange(tab_n + 1) * 1e-5, 1.9, 15.0).astype(np.float32)
        nf = np.float32(orc_rc.mkb_rl_r2(np.array([0.0]), 1.9, 15.0)[0])
        rng = np.random.default_rng(11)
        quad = orc_rc._ft_quad(vdim).astype(np.float64)
        T = np.ascontiguousarray(((50.0 / (1.0 + np.sqrt(quad))) * rng.uniform(0.8, 1.2, quad.shape)
                                  ).astype(np.float32))
        W = np.zeros_like(T)
        it = ctypes.c_int()
        check(L.thx_ExposeWT(0, P(T), P(W), P(tab), np.float32(1e-5), tab_n, nf, maxR, pf, vdim, 30, 10, N,
                             ctypes.byref(it)), "ExposeWT")
        return {"W": W, "T": T, "nIter": np.array(it.value)}
    out.append(("thx_ExposeWT N=32 pf=2", expose_wt))

    def translate():
        dim, r = 32, 12
        rng = np.random.default_rng(8)
        V = (rng.standard_normal((dim, dim, dim // 2 + 1))
             + 1j * rng.standard_normal((dim, dim, dim // 2 + 1))).astype(np.complex64)
        check(L.thx_TranslateI(0, P(V), -1.7, 2.25, 0.6, r, dim), "TranslateI")
        return {"V": V}
    out.append(("thx_TranslateI dim=32 r=12", translate))

    # ---- the particle statistics' entry points (csrc/optimiser.hip), on the
    # smallest clouds at which their shared pieces can go wrong: 33 images
    # (several per wave, the last wave part full); 8 lanes per image hold 16
    # particles each, so mR covers lanes with no particle, a part-full last
    # lane, the register path exactly full (128) and the strided path past it
    nI, MR, MT, MD = 33, (1, 7, 8, 9, 125, 128, 129, 200), (1, 2, 9, 151), (1, 2, 9)
    KINDS = ("3deg", "40deg", "runs", "equal")

    def cloud(kind, m, two_d):
        """[nI, m, 4] rotations: clustered at 3 / 40 degrees, a few ancestors
        repeated in sorted order (as a gather leaves them), or one repeated"""
        g = np.random.default_rng([77, m, KINDS.index(kind), int(two_d)])
        n = {"runs": min(m, 5), "equal": 1}.get(kind, m)
        spread = 40.0 if kind == "40deg" else 3.0
        if two_d:
            th = g.uniform(0, 2 * np.pi, (nI, 1)) + g.standard_normal((nI, n)) * np.radians(spread)
            q = np.stack([np.cos(th), np.sin(th), np.zeros_like(th), np.zeros_like(th)], axis=-1)
        else:
            q = synth.clustered_quaternions(nI, n, spread, g)
        idx = np.sort(g.integers(0, n, size=(nI, m)), axis=1)
        return np.take_along_axis(q, idx[..., None].repeat(4, -1), axis=1) if n < m else q

    def shifts(mT):
        return np.random.default_rng([78, mT]).standard_normal((nI, mT, 2)) * 2.0

    def f64(*shape):
        return torch.empty(*shape, dtype=torch.float64, device=dev)

    for two_d in (False, True):
        for m in MR:
            for kind in KINDS:
                def vari(two_d=two_d, m=m, kind=kind):
                    q, res = T_(cloud(kind, m, two_d)), {}
                    for mT in MT:
                        t = T_(shifts(mT))
                        if two_d:
                            k, sd = f64(nI, 3), f64(nI, 2)
                            check(L.thx_pf_calvari2d(nI, m, _ptr(q), mT, _ptr(t), 0.0, 0.0, _ptr(k),
                                                     _ptr(sd), None), "thx_pf_calvari2d")
                        else:
                            k, sd = ops.pf_calvari(q, t)
                        res[f"k mT={mT}"], res[f"sd mT={mT}"] = host(k), host(sd)
                    return res
                out.append((f"thx_pf_calvari{'2d' if two_d else ''} mR={m} {kind}", vari))

                def perturb(two_d=two_d, m=m, kind=kind):
                    c, res = cloud(kind, m, two_d), {}
                    k = T_(np.tile([0.02, 0.01, 0.03], (nI, 1)))
                    sd = T_(np.tile([1.5, 2.0], (nI, 1)))
                    for mT in MT:       # transM 4: some translations are re-centred
                        q, t = T_(c), T_(shifts(mT))
                        if two_d:
                            pR, pT = f64(nI, m), f64(nI, mT)
                            check(L.thx_pf_perturb2d(nI, m, mT, _ptr(q), _ptr(t), _ptr(pR), _ptr(pT),
                                                     _ptr(k), _ptr(sd), 1.0, 2.0, 4.0, SEED, 3, None),
                                  "thx_pf_perturb2d")
                        else:
                            pR, pT = ops.pf_perturb(q, t, T_(c[:, 0]), k, sd, 1.0, 2.0, 4.0, SEED, 3)
                        res.update({f"{n} mT={mT}": host(v)
                                    for n, v in (("quat", q), ("trans", t), ("pR", pR), ("pT", pT))})
                    return res
                out.append((f"thx_pf_perturb{'2d' if two_d else ''} mR={m} {kind}", perturb))

                if not two_d:
                    out.append((f"thx_pf_balance_rot mR={m} {kind}", lambda m=m, kind=kind: {
                        "pR": host(ops.pf_balance_rot(T_(cloud(kind, m, False))))}))

    for mD in MD:
        for kind in ("spread", "equal"):
            def defocus(mD=mD, kind=kind):
                g = np.random.default_rng([79, mD])
                d0 = 1.02 + (0.05 * g.standard_normal((nI, mD)) if kind == "spread" else np.zeros((nI, mD)))
                res = {}
                d, pD, sd = f64(nI, mD), f64(nI, mD), f64(nI)
                ops.pf_defocus("init", d, pD, arg=0.05, seed=SEED, stream_id=5)
                res["init d"], res["init pD"] = host(d), host(pD)
                d = T_(d0)
                ops.pf_defocus("vari", d, sd=sd)
                res["vari sd"] = host(sd)
                ops.pf_defocus("perturb", d, pD, sd, arg=0.7, seed=SEED, stream_id=6)
                res["perturb d"], res["perturb pD"] = host(d), host(pD)
                return res
            out.append((f"thx_pf_defocus ops 0, 2, 1 mD={mD} {kind}", defocus))
    return out


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dump(path, only=""):
    import torch
    if not torch.cuda.is_available():
        sys.exit("volume_identity: no GPU")
    saved = {}
    for name, thunk in rows():
        if not name.startswith(only):
            continue
        one, two = thunk(), thunk()
        torch.cuda.synchronize()
        rep = sorted(one) == sorted(two) and all(same(one[k], two[k]) for k in one)
        saved[f"{name}|repeat_identical"] = np.array(rep)
        for k, v in one.items():
            v = np.ascontiguousarray(v)
            if v.nbytes > BIG:      # its SHA-256 stands for a large tensor
                v = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8)
            saved[f"{name}|{k}"] = v
        print(json.dumps({"lib": os.path.basename(os.environ.get("THX_LIB", "prod")), "row": name,
                          "repeat_identical": bool(rep)}), flush=True)
    np.savez(path, **saved)


def compare(parent, child, out):
    p, c = np.load(parent), np.load(child)
    names = []
    for key in p.files:
        row = key.split("|")[0]
        if row not in names:
            names.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    bad = 0
    with open(out, "w") as f:
        for row in names:
            tensors = sorted(k.split("|", 1)[1] for k in p.files
                             if k.startswith(row + "|") and not k.endswith("|repeat_identical"))
            differ = [t for t in tensors if f"{row}|{t}" not in c.files
                      or not same(p[f"{row}|{t}"], c[f"{row}|{t}"])]
            rec = {"row": row, "tensors": tensors, "equal": not differ, "differing": differ,
                   "parent_repeat_identical": bool(p[f"{row}|repeat_identical"]),
                   "child_repeat_identical": bool(c[f"{row}|repeat_identical"])
                   if f"{row}|repeat_identical" in c.files else None}
            rec["in_verdict"] = rec["parent_repeat_identical"]
            bad += rec["in_verdict"] and not (rec["equal"] and rec["child_repeat_identical"])
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
    print(f"volume_identity: {len(names)} rows, {bad} defective")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_helpers_identity.jsonl"))
    ap.add_argument("--only", default="", help="dump the rows whose name starts with this")
    a = ap.parse_args()
    if a.dump:
        dump(a.dump, a.only)
    elif a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.out))
    else:
        ap.error("--dump or --compare")


if __name__ == "__main__":
    main()
