"""GPU parity of the product path at every BASELINE.json configuration that
fits one GPU:

  C2  box 128, nR 500 -> 1500 (the MIN_M_S clamp of src/Optimiser.cpp:170-175),
      nT 151, rU 12 (nPxl 211) / full-res rU 62 (nPxl 5 941);
  C3  box 256, nR 2000, nT 151, rU 24 (nPxl 870) -- the metric config -- with
      the product scan (algo 4, bf16x6 with the cancellation guard,
      160-column tiles) against the oracle over ALL 2000 x 151 samples, its
      per-sample dvp dumped (thx_global_scan_dvp, the element-wise
      dump-compare of gpu/src/cuthunder.cu:2247-2271) at SNR 0.05 and 20;
  C5  box 512, rL 3, full-res rU 254 (nPxl 100 928), local search mLR 200 x
      mLT 9, both volume layouts.

Tolerances: baselines (max dvp) 1e-5 relative; per-sample dvp 1e-5
relative (the north-star bar is 1e-4); scan marginals 1e-3 relative on
entries >= 1e-4 of the image maximum -- the oracle's own budget: its FP32
dvp sit ~2e-6 from the exact sum, which moves its marginals by up to 9e-4
(tests/test_parity_budget.py), and the product scan is held to the same
float64 budget (test_c3_scan_error_budget_against_float64); local-phase
marginals 1e-4 against a
float64 normalisation of the kernel's own dvp (the dvp themselves are held
to the oracle at 1e-5: one FP32 ulp of a dvp of magnitude |dvp| is
|dvp| * 6e-8 in log-weight, and full-resolution dvp reach 1e4-1e5)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from thunder_amd import expectation as ex
from thunder_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _marginals_close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = ref >= 1e-4 * ref.max(axis=-1, keepdims=True)
    rel = np.abs(got - ref)[m] / ref[m]
    assert rel.max() < tol, rel.max()


def _scan_vs_oracle(orc, vol, px, pxh, N, pf, gset, dat, ctf, sig, algo):
    q, t, pR, pT = gset
    rotP = ops.project3d(vol, ops.rotmat(T(q)), px)
    traP = ops.trans_table(T(t), px)
    wC, wR, wT, base = (x.cpu().numpy() for x in ops.global_scan(
        rotP, traP, dat, ctf, sig, T(pR), T(pT), algo=algo))
    d = orc.dvp_global(vol.cpu().numpy(), pf * N, pf, q, t, dat.cpu().numpy(), ctf.cpu().numpy(),
                       sig.cpu().numpy(), pxh, N, threads=16)
    rC, rR, rT, rb = orc.weights_global(d, pR, pT)
    nImg = dat.shape[0]
    assert np.allclose(base, rb, rtol=1e-5, atol=0), np.max(np.abs(base - rb) / np.abs(rb))
    _marginals_close(wR.reshape(nImg, -1), rR.reshape(nImg, -1), 1e-3)
    _marginals_close(wT.reshape(nImg, -1), rT.reshape(nImg, -1), 1e-3)
    assert np.allclose(wC.reshape(-1), rC, rtol=1e-3, atol=0)


def _phase_vs_oracle(orc, vol, px, pxh, N, pf, quat, trans, dat, ctf, sig, cells=None, tol=1e-5,
                     ypair=None, routed=False, ball=None, ball_r=0):
    """The phase in the given layout (routed: thx_local_phase_routed, whose
    kernel choice is returned) against orc.local_phase image by image."""
    nImg, mR = quat.shape[:2]
    mT = trans.shape[1]
    pR = np.full((nImg, mR), 1.0 / mR)
    pT = np.full((nImg, mT), 1.0 / mT)
    out = ops.local_phase(vol, T(quat), T(trans), T(np.ones(nImg)), T(pR), T(pT), dat, ctf, sig, px,
                          want_dvp=True, cells=cells, ypair=ypair, routed=routed, ball=ball,
                          ball_r=ball_r)
    wC, wR, wT, base, d = out[:5]
    d, wR, wT, base = d.cpu().numpy(), wR.cpu().numpy(), wT.cpu().numpy(), base.cpu().numpy()
    vnp = vol.cpu().numpy()
    for l in range(nImg):
        rC, rR, rT, rb, rd = orc.local_phase(vnp, pf * N, pf, quat[l], trans[l], 1.0, pR[l], pT[l],
                                             dat[l].cpu().numpy(), ctf[l].cpu().numpy(),
                                             sig[l].cpu().numpy(), pxh, N)
        assert np.max(np.abs(d[l] - rd) / np.abs(rd)) < tol
        assert abs(base[l] - rb) <= 1e-5 * abs(rb)
        # the normalisation (src/Optimiser.cpp:1383-1402) checked on the
        # kernel's own dvp: a weight exp(dvp - base) moves by the dvp's FP32
        # summation error (|dvp| reaches 1e4-1e5 at full resolution, where one
        # part in 1e7 is already 1e-3 in log-weight), which the dvp bound above
        # covers; here only the marginals' arithmetic is compared, in float64
        e = np.exp(d[l].astype(np.float64) - d[l].max())
        _marginals_close(wR[l], e @ pT[l], 1e-4)
        _marginals_close(wT[l], pR[l] @ e, 1e-4)
    return out[5] if routed else None


# ---------------------------------------------------------------------- C3
@pytest.fixture(scope="module")
def c3():
    from bench import make_stack
    N, pf = 256, 2
    vol = synth.projectee(synth.blob_volume(N, seed=1, device=DEV), pf)
    px, dat, ctf, sig, *_ = make_stack(N, pf, 24, 1, 16, DEV, seed=19, vol=vol)
    return dict(N=N, pf=pf, vol=vol, px=px, dat=dat, ctf=ctf, sig=sig)


def test_c3_product_scan_matches_oracle(orc, c3):
    """algo 4 (bf16x6, the product path) on ALL 2000 rotations x 151
    translations x 16 images against the restatement's weights."""
    gset = synth.global_sample_set(2000, seed=2)
    pxh = orc.pixel_set(256, 2, 24, 1)
    assert pxh.n == 870 and len(gset[1]) == 151
    _scan_vs_oracle(orc, c3["vol"], c3["px"], pxh, 256, 2, gset, c3["dat"], c3["ctf"], c3["sig"],
                    algo=4)


@pytest.mark.parametrize("snr", [0.05, 20.0])
@pytest.mark.parametrize("algo", [4, 2])
def test_c3_product_scan_dvp_per_sample(orc, c3, snr, algo):
    """Every sample's log-likelihood of the product scan, dumped by
    thx_global_scan_dvp, against orc.dvp_global (src/Optimiser.cpp:9187-9213)
    over ALL 2000 x 151 samples of 8 images at 1e-5 relative, at the bench's
    SNR 0.05 and at SNR 20 (images at grid poses).  At SNR 20 the expanded
    form dvp = A + B + X cancels ~80x at the true pose; without the guard the
    FP32 accumulation of X misses 1e-5 there (checked below), with it the
    flagged samples are recomputed in the direct form.  The marginals are the
    float64 normalisation of the dumped dvp to 1e-4 (the dvp themselves carry
    the FP32 summation error, |dvp| * ~1e-6, which moves a weight by as much),
    the baseline its max exactly."""
    from test_gpu_driver import grid_images
    gset = q, t, pR, pT = synth.global_sample_set(2000, seed=2)
    pxh = orc.pixel_set(256, 2, 24, 1)
    vol, px, n = c3["vol"], c3["px"], 8
    if snr < 1:
        dat, ctf, sig = (c3[k][:n].contiguous() for k in ("dat", "ctf", "sig"))
    else:
        dat, ctf, sig = grid_images(vol[None].contiguous(), px, gset, n, seed=70, snr=snr)[:3]
    rotP = ops.project3d(vol, ops.rotmat(T(q)), px)
    traP = ops.trans_table(T(t), px)
    ref = orc.dvp_global(vol.cpu().numpy(), 512, 2, q, t, dat.cpu().numpy(), ctf.cpu().numpy(),
                         sig.cpu().numpy(), pxh, 256, threads=16).astype(np.float64)
    wC, wR, wT, base, d = (x.cpu().numpy() for x in ops.global_scan(
        rotP, traP, dat, ctf, sig, T(pR), T(pT), algo=algo, want_dvp=True))
    rel = np.abs(d - ref) / np.abs(ref)
    assert rel.max() < 1e-5, (rel.max(), np.unravel_index(rel.argmax(), rel.shape))
    d64 = d.astype(np.float64).reshape(n, -1)
    assert np.array_equal(base, d.reshape(n, -1).max(1))
    e = np.exp(d64 - d64.max(1, keepdims=True)).reshape(n, len(q), len(t))
    _marginals_close(wR.reshape(n, -1), e @ pT, 1e-4)
    _marginals_close(wT.reshape(n, -1), np.einsum("lrt,r->lt", e, pR), 1e-4)
    assert np.allclose(wC.reshape(-1), np.einsum("lrt,r,t->l", e, pR, pT), rtol=1e-4, atol=0)
    if snr > 1 and algo == 4:
        # the guard is what holds 1e-5 here: off, the expansion misses it
        d0 = ops.global_scan(rotP, traP, dat, ctf, sig, T(pR), T(pT), algo=algo, guard=0.0,
                             want_dvp=True)[4].cpu().numpy()
        assert (np.abs(d0 - ref) / np.abs(ref)).max() > 1e-5


@pytest.mark.parametrize("snr", [0.05, 20.0])
def test_c3_scan_error_budget_against_float64(orc, c3, snr):
    """The product scan's own error against the exact sum: every sample's dvp
    (thx_global_scan_dvp) of 120 of the 2000 rotations x all 151
    translations x 3 images against a float64 evaluation of the direct form
    from the same FP32 tables (the GPU's P and T), and the marginals of both.
    The same budget as the oracle's own FP32 evaluation
    (tests/test_parity_budget.py: dvp within 5e-6 of float64, marginals
    within 1e-3), so the GPU is held to the exact sum at least as tightly as
    the restatement it is compared with."""
    from test_parity_budget import c3_budget_stack, dvp_float64, marginals, max_marginal_rel
    q, t, pR, pT = synth.global_sample_set(2000, seed=2)
    rsel = np.sort(np.random.default_rng(5).choice(2000, 120, replace=False))
    pxh = orc.pixel_set(256, 2, 24, 1)
    dat, ctf, sig = c3_budget_stack(orc, c3["vol"].cpu().numpy(), pxh, (q, t, pR, pT), rsel, snr, 3, 70)
    rotP = ops.project3d(c3["vol"], ops.rotmat(T(q[rsel])), c3["px"])
    traP = ops.trans_table(T(t), c3["px"])
    pRs = np.full(len(rsel), 1.0 / len(rsel))
    d = ops.global_scan(rotP, traP, T(dat), T(ctf), T(sig), T(pRs), T(pT), algo=4,
                        want_dvp=True)[4].cpu().numpy().astype(np.float64)
    ref = dvp_float64(rotP.cpu().numpy(), traP.cpu().numpy(), dat, ctf, sig)
    rel = np.abs(d - ref) / np.abs(ref)
    assert rel.max() < 5e-6, rel.max()
    wR, wT = marginals(d, pRs, pT)
    rR, rT = marginals(ref, pRs, pT)
    mr = max(max_marginal_rel(wR, rR), max_marginal_rel(wT, rT))
    assert mr < 1e-3, mr


def test_c3_fp32_scan_matches_oracle(orc, c3):
    gset = synth.global_sample_set(2000, seed=2)
    pxh = orc.pixel_set(256, 2, 24, 1)
    n = 4
    _scan_vs_oracle(orc, c3["vol"], c3["px"], pxh, 256, 2, gset, c3["dat"][:n].contiguous(),
                    c3["ctf"][:n].contiguous(), c3["sig"][:n].contiguous(), algo=1)


@pytest.mark.parametrize("layout", ["halfcomplex", "ypair", "routed", "ball"])
def test_c3_local_phase_bench_clouds_match_oracle(orc, c3, layout):
    """The half-complex layout, the pair-form y-pair kernel (the one every
    bench phase runs), the device route with a y-pair copy and the route on
    the driver's compact ball (thx_local_phase_routed_ball: the copy the bench
    gathers from, R = ceil(pf r_max) + 2 = 49 at rU 24) at the bench's cloud
    widths (3, 10 and 30 degrees), 125 x 9: dvp 1e-5 against the oracle; the
    route takes the y-pair kernel for the wide clouds."""
    rng = np.random.default_rng(8)
    pxh = orc.pixel_set(256, 2, 24, 1)
    yp = ops.volume_ypair(c3["vol"]) if layout in ("ypair", "routed") else None
    kw = {}
    if layout == "ball":
        R = ops.ypair_ball_radius(c3["px"])
        assert R == 49
        kw = dict(ball=ops.volume_ypair_ball(c3["vol"], R), ball_r=R)
    for spread in (3.0, 10.0, 30.0):
        quat = synth.clustered_quaternions(16, 125, spread, rng)
        trans = rng.standard_normal((16, 9, 2)) * 2
        r = _phase_vs_oracle(orc, c3["vol"], c3["px"], pxh, 256, 2, quat, trans, c3["dat"], c3["ctf"],
                             c3["sig"], ypair=yp, routed=layout in ("routed", "ball"), **kw)
        if layout in ("routed", "ball") and spread >= 10:
            assert r == 2, (spread, r)


def test_ball_at_high_resolution_matches_oracle(orc, c3):
    """The compact ball where it is largest and still smaller than the
    volume: box 256, rU 100 (nPxl 15.6k, R = 203 of the 257 x-columns), 1.5
    and 3 degree clouds -- thx_local_phase_routed_ball against the oracle at
    1e-5.  (At the full-resolution radius rU 126 the ball would be the whole
    volume, so the driver passes the whole y-pair copy, covered by
    test_gpu_fullsize / the C5 test.)"""
    from bench import make_stack
    px, dat, ctf, sig, *_ = make_stack(256, 2, 100, 1, 4, DEV, seed=33, vol=c3["vol"])
    pxh = orc.pixel_set(256, 2, 100, 1)
    R = ops.ypair_ball_radius(px)
    assert R + 2 <= 257 and px.n > 15000
    ball = ops.volume_ypair_ball(c3["vol"], R)
    rng = np.random.default_rng(9)
    for spread in (1.5, 3.0):
        quat = synth.clustered_quaternions(4, 125, spread, rng)
        trans = rng.standard_normal((4, 9, 2))
        r = _phase_vs_oracle(orc, c3["vol"], px, pxh, 256, 2, quat, trans, dat, ctf, sig, routed=True,
                             ball=ball, ball_r=R)
        assert r in (0, 2)


def test_ball_rejects_a_radius_the_ring_does_not_fit(c3):
    """pf r_max + 2 > ballR would gather outside the ball: refused before any
    launch (thx_local_phase_routed_ball reads the ring radius back)."""
    R = ops.ypair_ball_radius(c3["px"])
    ball = ops.volume_ypair_ball(c3["vol"], R - 1)
    one = lambda *sh: torch.ones(*sh, dtype=torch.float64, device=DEV)
    q = T(synth.clustered_quaternions(2, 8, 3.0, np.random.default_rng(1)))
    t = torch.zeros(2, 3, 2, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="needs ballR"):
        ops.local_phase(c3["vol"], q, t, one(2), one(2, 8), one(2, 3), c3["dat"][:2].contiguous(),
                        c3["ctf"][:2].contiguous(), c3["sig"][:2].contiguous(), c3["px"],
                        routed=True, ball=ball, ball_r=R - 1)


def test_c3_driver_routes_bench_phases_to_ypair(c3):
    """thx_expectation at the bench's configuration (C3, nR 2000 x 151, 10
    phases of 125 x 9) on 512 images: the device route's choice per phase
    (thx_expect_cfg.phaseRoute) is the pair-form y-pair kernel in every phase,
    the kernel the bench's roofline line prices."""
    from bench import make_stack
    px, dat, ctf, sig, *_ = make_stack(256, 2, 24, 1, 512, DEV, seed=5, vol=c3["vol"])
    e = ex.Expectation(c3["vol"], px, synth.global_sample_set(2000, seed=2), n_phase=10, seed=3)
    routes = e.track_routes(10)
    e.run(dat, ctf, sig)
    assert routes.cpu().tolist() == [2] * 10, routes.cpu().tolist()


# ------------------------------------------------ one phase, five entry points
def _phase_tile_rotations():
    """RT of local.hip: the rotations one workgroup of the phase kernel covers."""
    src = open(os.path.join(os.path.dirname(ops.__file__), "csrc", "local.hip")).read()
    threads = int(re.search(r"constexpr int THREADS = (\d+);", src).group(1))
    assert re.search(r"constexpr int NWAVE = THREADS / 64;", src)
    assert re.search(r"constexpr int RT = 16 \* NWAVE;", src)
    return 16 * (threads // 64)


class _LocalSel(ctypes.Structure):      # thx_local_sel
    _fields_ = [("active", ctypes.c_void_p), ("nActive", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("volStride", ctypes.c_longlong)]


@pytest.mark.parametrize("tiles", [1, 2])
def test_entry_points_of_one_phase_agree_bitwise(tiles):
    """The entry points that describe the same phase run the same launches:
    thx_local_phase (layout 0, pxOrder), thx_local_phase_sel with an all-null
    sel and thx_local_phase_routed without a y-pair copy agree bit for bit on
    wC, wR, wT, baseL and dvp, and so do thx_local_phase_routed on the whole
    y-pair copy and thx_local_phase_routed_ball on the matching ball, which
    also report the same route.  Box 32, 3 images, nT 3; nR 5 is one workgroup
    per image with the fused epilogue, nR = RT + 1 two rotation tiles with the
    likelihoods materialised and k_local_weights after them.  Each with a 1
    degree cloud, whose patch boxes fit the LDS (route 0: the staged kernel),
    and with unrelated rotations, under which a patch's copies span the ring's
    whole shell and most boxes do not fit (route 1 box-less / 2 y-pair) --
    with nR = RT + 1 the second tile's single rotation makes its boxes fit,
    which is half the sampled patches, so the route stays staged at its 50 per
    cent threshold and the other kernel, launched all the same, exits at entry.
    The phases are run-to-run deterministic
    (profiles/driver_refactor_identity.jsonl), hence equality, no tolerance."""
    from bench import make_stack
    from thunder_amd._lib import check, lib
    N, pf, nImg, nT = 32, 2, 3, 3
    nR = 5 if tiles == 1 else _phase_tile_rotations() + 1
    vol = synth.projectee(synth.blob_volume(N, seed=7, device=DEV), pf)
    px, dat, ctf, sig, *_ = make_stack(N, pf, 12, 1, nImg, DEV, seed=61, vol=vol)
    yp, R = ops.volume_ypair(vol), ops.ypair_ball_radius(px)
    ball = ops.volume_ypair_ball(vol, R)
    rng = np.random.default_rng(14)
    trans = T(rng.standard_normal((nImg, nT, 2)))
    pC, pR, pT = T(np.ones(nImg)), T(np.full((nImg, nR), 1.0 / nR)), T(np.full((nImg, nT), 1.0 / nT))
    ws = ops.workspace(lib().thx_local_phase_workspace(nImg, nR, nT, len(px.order)), DEV)
    p, sel = ops._ptr, _LocalSel(None, None, None, 0)

    def run(fn, lead, quat, routed):
        out = [torch.full(sh, float("nan"), dtype=torch.float32, device=DEV)
               for sh in ((nImg,), (nImg, nR), (nImg, nT), (nImg,), (nImg, nR, nT))]
        route = torch.full((1,), -2, dtype=torch.int32, device=DEV)
        check(getattr(lib(), fn)(
            *lead, pf * N, pf, p(quat), nR, p(trans), nT, p(pC), p(pR), p(pT), p(dat), p(ctf), p(sig),
            p(px.d_iCol), p(px.d_iRow), p(px.d_order), len(px.order), px.n, px.idim, nImg,
            *(p(x) for x in out), *((p(route),) if routed else ()), p(ws), ws.numel(),
            ops._stream(DEV)), fn)
        assert all(bool(torch.isfinite(x).all()) for x in out), fn
        return [x.view(torch.int32) for x in out], int(route.item())

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    routes = []
    for quat in (T(synth.clustered_quaternions(nImg, nR, 1.0, rng)),
                 T(synth.uniform_quaternions(nImg * nR, rng).reshape(nImg, nR, 4))):
        plain, _ = run("thx_local_phase", (p(vol), 0), quat, False)
        by_sel, _ = run("thx_local_phase_sel", (ctypes.addressof(sel), p(vol), 0), quat, False)
        routed, r0 = run("thx_local_phase_routed", (None, p(vol), None), quat, True)
        assert same(plain, by_sel) and same(plain, routed)
        whole, r1 = run("thx_local_phase_routed", (None, p(vol), p(yp)), quat, True)
        compact, r2 = run("thx_local_phase_routed_ball", (None, p(vol), p(ball), R), quat, True)
        assert same(whole, compact) and r1 == r2
        routes.append((r0, r1))
    assert routes == [(0, 0), (1, 2) if tiles == 1 else (0, 0)], routes


# ---------------------------------------------------------------------- C2
@pytest.fixture(scope="module")
def c2():
    from bench import make_stack
    N, pf = 128, 2
    vol = synth.projectee(synth.blob_volume(N, seed=3, device=DEV), pf)
    px, dat, ctf, sig, *_ = make_stack(N, pf, 12, 0, 32, DEV, seed=23, vol=vol)
    return dict(N=N, pf=pf, vol=vol, px=px, dat=dat, ctf=ctf, sig=sig)


def test_c2_sample_set_sizes():
    """mS = 500 is clamped to MIN_M_S = 1500 (src/Optimiser.cpp:170-175,
    include/Optimiser.h:50) for 3D C1: nR = mS / (1 + nSym) = 1500."""
    MIN_M_S = 1500
    nR = max(500, MIN_M_S * (1 + 0)) // (1 + 0)
    assert nR == 1500 and synth.n_trans_global() == 151


@pytest.mark.parametrize("algo", [1, 2])
def test_c2_scan_matches_oracle(orc, c2, algo):
    gset = synth.global_sample_set(1500, seed=4)
    pxh = orc.pixel_set(128, 2, 12, 0)
    assert pxh.n == 211
    _scan_vs_oracle(orc, c2["vol"], c2["px"], pxh, 128, 2, gset, c2["dat"], c2["ctf"], c2["sig"],
                    algo=algo)


@pytest.mark.parametrize("cells", [False, True])
def test_c2_full_resolution_phase_matches_oracle(orc, c2, cells):
    from bench import make_stack
    px, dat, ctf, sig, *_ = make_stack(128, 2, 62, 0, 3, DEV, seed=29, vol=c2["vol"])
    assert px.n == 5941
    pxh = orc.pixel_set(128, 2, 62, 0)
    rng = np.random.default_rng(2)
    quat = synth.clustered_quaternions(3, 125, 5.0, rng)
    trans = rng.standard_normal((3, 9, 2))
    cl = ops.volume_cells(c2["vol"]) if cells else None
    _phase_vs_oracle(orc, c2["vol"], px, pxh, 128, 2, quat, trans, dat, ctf, sig, cells=cl)


def test_c2_expectation_recovers_grid_poses(c2):
    """thx_expectation end to end at C2 (box 128, nR 1500, nT 151, rU 12,
    10 phases of 125 x 9): images made at grid poses at high SNR keep the
    cloud on the generating pose; the particle state is well formed."""
    N, pf = 128, 2
    px = c2["px"]
    gset = synth.global_sample_set(1500, seed=4)
    q, t, pR, pT = gset
    rng = np.random.default_rng(41)
    nImg = 256
    ir = rng.integers(0, len(q), nImg)
    near = np.argsort(np.linalg.norm(t, axis=1))[:40]
    it = near[rng.integers(0, len(near), nImg)]
    qtrue, ttrue = T(q[ir]), T(t[it])
    ctf = ops.ctf(T(synth.ctf_attrs(nImg, seed=42)), px)
    sigl = ctf * ops.project3d(c2["vol"], ops.rotmat(qtrue), px) * ops.trans_table(ttrue, px)
    dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=20.0, seed=43)
    e = ex.Expectation(c2["vol"], px, gset, n_phase=10, seed=3)
    quat, trans, pRo, pTo, score = e.run(dat, ctf, sig)[:5]
    c = (ex.cloud_mode(quat) * qtrue).sum(-1).abs().clamp(max=1)
    err = torch.rad2deg(2 * torch.acos(c))
    assert float(err.median()) < 2.0 and float((err > 10).double().mean()) <= 0.05
    assert torch.isfinite(quat).all() and torch.isfinite(score).all()
    assert torch.allclose(quat.norm(dim=-1), torch.ones_like(quat[..., 0]), atol=1e-9)
    assert torch.allclose(pRo.sum(-1), torch.ones_like(pRo[:, 0]), rtol=1e-9)


# ---------------------------------------------------------------------- C5
@pytest.fixture(scope="module")
def c5():
    from bench import make_stack
    N, pf = 512, 2
    vol = synth.projectee(synth.blob_volume(N, seed=5, device=DEV), pf)
    px, dat, ctf, sig, *_ = make_stack(N, pf, 254, 3, 2, DEV, seed=31, vol=vol)
    yield dict(N=N, pf=pf, vol=vol, px=px, dat=dat, ctf=ctf, sig=sig)
    del vol
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", ["halfcomplex", "cells", "ypair"])
def test_c5_full_resolution_local_search_matches_oracle(orc, c5, layout):
    """Large-box stress: box 512 (projectee 4.3 GB, cells 34 GB, y-pairs
    8.6 GB), nPxl 100 928, mLR 200 x mLT 9 local-search clouds of 2 degrees."""
    px = c5["px"]
    assert px.n == 100928
    pxh = orc.pixel_set(512, 2, 254, 3)
    rng = np.random.default_rng(12)
    quat = synth.clustered_quaternions(2, 200, 2.0, rng)
    trans = rng.standard_normal((2, 9, 2))
    cl = ops.volume_cells(c5["vol"]) if layout == "cells" else None
    yp = ops.volume_ypair(c5["vol"]) if layout == "ypair" else None
    # tol: the north-star 1e-4 -- both sides sum 100 928 FP32 terms, the
    # oracle strictly in order (error growing ~ n eps), so 1e-5 is within the
    # oracle's own rounding at this length (measured 1.7e-5)
    _phase_vs_oracle(orc, c5["vol"], px, pxh, 512, 2, quat, trans, c5["dat"], c5["ctf"],
                     c5["sig"], cells=cl, ypair=yp, tol=1e-4)
    del cl, yp
    torch.cuda.empty_cache()
