"""GPU parity: every HIP kernel of the C-ABI against the CPU restatement.

Tolerances (written here, per north_star "within 1e-4 relative"):
  * integer / index work (pixel set, resample ancestors, counter): bit-exact;
  * per-particle log-likelihoods dvp: 1e-5 relative (bar: 1e-4);
  * projections / phase tables / CTF: FP32 rounding of the reference formula;
  * marginal weights exp(dvp - base): 1e-3 relative on entries >= 1e-4 of the
    image maximum (one FP32 ulp of a dvp of magnitude |dvp| moves a weight by
    ~|dvp| * 6e-8 relative), normalisations and baselines 1e-5;
  * half-map F / T after atomic scatter: 1e-5 of max|F| (summation order is
    not reproducible on either side), FSC 1e-6 absolute.
"""
import ctypes

import numpy as np
import pytest
import torch

from stacks import np_dvp, small_stack
from thunder_amd import ops, synth
from thunder_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope="module")
def stack(orc):
    return small_stack(orc, N=32, nImg=8, nR=12, nT=11, seed=3)


def dev_pixels(s):
    px = ops.PixelSet(s["N"], s["pf"], s["rU"], s["rL"], device=DEV)
    assert np.array_equal(px.iCol, s["px"].iCol) and np.array_equal(px.iRow, s["px"].iRow)
    return px


def test_ctf_trans_rotmat(orc, stack):
    s = stack
    px = dev_pixels(s)
    attrs = synth.ctf_attrs(5, seed=8)
    got = ops.ctf(T(attrs), px).cpu().numpy()
    for l, a in enumerate(attrs):
        assert np.max(np.abs(got[l] - orc.ctf(s["px"], a, s["N"]))) < 5e-5
    tr = np.array([[0.0, 0.0], [3.3, -2.1], [-9.75, 12.5]])
    gt = ops.trans_table(T(tr), px).cpu().numpy()
    for t in range(3):
        assert np.max(np.abs(gt[t] - orc.translate(s["px"], tr[t, 0], tr[t, 1], s["N"]))) < 2e-5
    q = synth.uniform_quaternions(7, np.random.default_rng(2))
    m = ops.rotmat(T(q)).cpu().numpy()
    for r in range(7):
        assert np.allclose(m[r], orc.rotate3d(q[r]), atol=1e-15, rtol=0)


def test_project3d(orc, stack):
    s = stack
    px = dev_pixels(s)
    vol = T(s["vol"])
    mat = np.stack([orc.rotate3d(q) for q in s["quat"]])
    got = ops.project3d(vol, T(mat), px).cpu().numpy()
    for r in range(len(mat)):
        ref = orc.project3d(s["vol"], s["vdim"], s["pf"], mat[r], s["px"])
        assert np.max(np.abs(got[r] - ref)) <= 1e-5 * np.max(np.abs(ref))


def gpu_tables(orc, s, px):
    mat = ops.rotmat(T(s["quat"]))
    rotP = ops.project3d(T(s["vol"]), mat, px)
    traP = ops.trans_table(T(s["trans"]), px)
    return rotP, traP


def test_dvp_direct(orc, stack):
    s = stack
    px = dev_pixels(s)
    rotP, traP = gpu_tables(orc, s, px)
    d = ops.dvp(rotP, traP, T(s["dat"]), T(s["ctf"]), T(s["sig"])).cpu().numpy()
    ref = orc.dvp_global(s["vol"], s["vdim"], s["pf"], s["quat"], s["trans"], s["dat"], s["ctf"],
                         s["sig"], s["px"], s["N"])
    assert np.max(np.abs(d - ref) / np.abs(ref)) < 1e-5


def check_weights(got, ref, nR, nT, rtol_base=1e-5, rtol_w=1e-3):
    wC, wR, wT, base = [x.cpu().numpy() for x in got]
    rC, rR, rT, rb = ref
    assert np.allclose(base, rb, rtol=rtol_base, atol=0)
    rR = rR.reshape(wR.shape)
    rT = rT.reshape(wT.shape)
    rC = rC.reshape(wC.shape)
    for a, b in ((wR, rR), (wT, rT), (wC, rC)):
        m = b >= 1e-4 * b.max(axis=-1, keepdims=True)
        assert np.all(np.abs(a - b)[m] <= rtol_w * b[m]), np.max(np.abs(a - b)[m] / b[m])
        assert np.allclose(a.sum(-1), b.sum(-1), rtol=min(1e-4 * rtol_w / 1e-3, 1e-2))


def scan_tol(algo):
    """every algorithm (0 direct, 1 FP32 MFMA, 2 bf16x3, 4 bf16x6) holds the
    baseline to 1e-5 and the marginals to 1e-3 against the restatement's."""
    return {}


@pytest.mark.parametrize("algo", [0, 1, 2, 4])
def test_global_scan(orc, stack, algo):
    s = stack
    px = dev_pixels(s)
    rotP, traP = gpu_tables(orc, s, px)
    nR, nT = len(s["quat"]), len(s["trans"])
    pR = np.full(nR, 1.0 / nR)
    pT = np.random.default_rng(1).uniform(0.2, 1.0, nT)
    pT /= pT.sum()
    got = ops.global_scan(rotP, traP, T(s["dat"]), T(s["ctf"]), T(s["sig"]), T(pR), T(pT),
                          algo=algo)
    dref = orc.dvp_global(s["vol"], s["vdim"], s["pf"], s["quat"], s["trans"], s["dat"],
                          s["ctf"], s["sig"], s["px"], s["N"])
    check_weights(got, orc.weights_global(dref, pR, pT), nR, nT, **scan_tol(algo))


@pytest.mark.parametrize("algo", [0, 1, 2, 4])
def test_global_scan_two_classes(orc, stack, algo):
    """kIdx > 0 merges into the running baseline (kernel_setBaseLine)."""
    s = stack
    px = dev_pixels(s)
    nR, nT = len(s["quat"]), len(s["trans"])
    pR = np.full(nR, 1.0 / nR)
    pT = np.full(nT, 1.0 / nT)
    vol2 = (s["vol"] * 1.3).astype(np.complex64)
    state = None
    ostate = None
    for k, v in enumerate((s["vol"], vol2)):
        rotP = ops.project3d(T(v), ops.rotmat(T(s["quat"])), px)
        traP = ops.trans_table(T(s["trans"]), px)
        state = ops.global_scan(rotP, traP, T(s["dat"]), T(s["ctf"]), T(s["sig"]), T(pR), T(pT),
                                kIdx=k, nK=2, state=state, algo=algo)
        d = orc.dvp_global(v, s["vdim"], s["pf"], s["quat"], s["trans"], s["dat"], s["ctf"],
                           s["sig"], s["px"], s["N"])
        ostate = orc.weights_global(d, pR, pT, kIdx=k, nK=2, state=ostate)
    check_weights(state, ostate, nR, nT, **scan_tol(algo))


def test_local_phase(orc, stack):
    s = stack
    px = dev_pixels(s)
    nImg, nR, nT = 5, 10, 9
    rng = np.random.default_rng(11)
    quat = synth.uniform_quaternions(nImg * nR, rng).reshape(nImg, nR, 4)
    trans = rng.standard_normal((nImg, nT, 2)) * 2
    pC = rng.uniform(0.5, 1, nImg)
    pR = rng.uniform(0.1, 1, (nImg, nR))
    pT = rng.uniform(0.1, 1, (nImg, nT))
    wC, wR, wT, base, d = ops.local_phase(T(s["vol"]), T(quat), T(trans), T(pC), T(pR), T(pT),
                                          T(s["dat"][:nImg]), T(s["ctf"][:nImg]),
                                          T(s["sig"][:nImg]), px, want_dvp=True)
    wC, wR, wT, base, d = [x.cpu().numpy() for x in (wC, wR, wT, base, d)]
    for l in range(nImg):
        rc, rr, rt, rb, rd = orc.local_phase(s["vol"], s["vdim"], s["pf"], quat[l], trans[l],
                                             pC[l], pR[l], pT[l], s["dat"][l], s["ctf"][l],
                                             s["sig"][l], s["px"], s["N"])
        assert np.max(np.abs(d[l] - rd) / np.abs(rd)) < 1e-5
        assert abs(base[l] - rb) <= 1e-5 * abs(rb)
        for a, b in ((wR[l], rr), (wT[l], rt)):
            m = b >= 1e-4 * b.max()
            assert np.all(np.abs(a - b)[m] <= 1e-3 * b[m])
        assert abs(wC[l] - rc) <= 1e-3 * rc


def test_local_phase_cells_layout_and_many_rotations(orc, stack):
    """The cell-expanded projectee gives the same taps and weights (each
    sample's 8 taps summed as a quad tree instead of in sequence, so equal
    to FP32 rounding); mR > 128 and mT > 16 exercise the multi-tile grid."""
    s = stack
    px = dev_pixels(s)
    nImg, nR, nT = 2, 150, 20
    rng = np.random.default_rng(12)
    quat = synth.uniform_quaternions(nImg * nR, rng).reshape(nImg, nR, 4)
    trans = rng.standard_normal((nImg, nT, 2)) * 2
    pC = np.ones(nImg)
    pR = np.full((nImg, nR), 1.0 / nR)
    pT = np.full((nImg, nT), 1.0 / nT)
    vol = T(s["vol"])
    cells = ops.volume_cells(vol)
    args = (T(quat), T(trans), T(pC), T(pR), T(pT), T(s["dat"][:nImg]), T(s["ctf"][:nImg]),
            T(s["sig"][:nImg]), px)
    a = ops.local_phase(vol, *args, want_dvp=True)
    b = ops.local_phase(vol, *args, want_dvp=True, cells=cells)
    da, db = a[4].cpu().numpy(), b[4].cpu().numpy()
    assert np.max(np.abs(da - db) / np.abs(da)) < 2e-6
    d = db
    for l in range(nImg):
        *_, rd = orc.local_phase(s["vol"], s["vdim"], s["pf"], quat[l], trans[l], 1.0, pR[l],
                                 pT[l], s["dat"][l], s["ctf"][l], s["sig"][l], s["px"], s["N"])
        assert np.max(np.abs(d[l] - rd) / np.abs(rd)) < 1e-5


def staged_fraction(orc, px, quat, pf, cap=6400):
    """Host restatement of the kernel's patch-neighbourhood bound: share of
    (image, patch) stages whose two folded boxes fit in the LDS capacity."""
    fits = []
    for q in quat:
        R = np.stack([orc.rotate3d(x) for x in q])              # column-major 3x3 -> [r, 9]
        R = R.reshape(-1, 3, 3).transpose(0, 2, 1)              # row-major
        for g in px.order.reshape(-1, 16):
            g = g[g >= 0]
            c = np.array([[a, b, 0.0] for b in (px.iRow[g].min(), px.iRow[g].max())
                          for a in (px.iCol[g].min(), px.iCol[g].max())]) * pf
            P = np.einsum("rij,kj->rki", R, c)                 # [r, 4, 3]
            mn, mx = P.min(1), P.max(1)
            tot = 0
            pos, neg = mx[:, 0] >= -1e-3, mn[:, 0] < 1e-3
            if pos.any():
                lo = np.floor(np.maximum(mn[pos], [0, -np.inf, -np.inf])).min(0) - 1
                hi = np.floor(mx[pos]).max(0) + 2
                lo[0] = max(lo[0], 0)
                tot += np.prod(hi - lo + 1)
            if neg.any():
                lo = np.floor(np.maximum(-mx[neg], [0, -np.inf, -np.inf])).min(0) - 1
                hi = np.floor(-mn[neg]).max(0) + 2
                lo[0] = max(lo[0], 0)
                tot += np.prod(hi - lo + 1)
            fits.append(tot <= cap)
    return float(np.mean(fits))


@pytest.fixture(scope="module")
def stack64(orc):
    return small_stack(orc, N=64, nImg=4, nR=4, nT=3, seed=4)


@pytest.mark.parametrize("spread,lo,hi", [(1.0, 0.99, 1.0), (8.0, 0.1, 0.6), (20.0, 0.0, 0.2)])
def test_local_phase_staged_patches(orc, stack64, spread, lo, hi):
    """Particle clouds of a few degrees: the tile-ordered kernel stages most
    16-pixel patch neighbourhoods in LDS, wide clouds fall back to direct
    gathers; both routes match the oracle and the set-order kernel."""
    s = stack64
    px = dev_pixels(s)
    nImg, nR, nT = 4, 125, 9
    rng = np.random.default_rng(13)
    quat = synth.clustered_quaternions(nImg, nR, spread, rng)
    frac = staged_fraction(orc, px, quat, s["pf"])
    assert lo <= frac <= hi, frac
    trans = rng.standard_normal((nImg, nT, 2)) * 2
    pC = np.ones(nImg)
    pR = np.full((nImg, nR), 1.0 / nR)
    pT = np.full((nImg, nT), 1.0 / nT)
    vol = T(s["vol"])
    args = (T(quat), T(trans), T(pC), T(pR), T(pT), T(s["dat"][:nImg]), T(s["ctf"][:nImg]),
            T(s["sig"][:nImg]), px)
    a = ops.local_phase(vol, *args, want_dvp=True)
    b = ops.local_phase(vol, *args, want_dvp=True, tiled=False)
    c = ops.local_phase(vol, *args, want_dvp=True, cells=ops.volume_cells(vol))
    assert np.max(np.abs(c[4].cpu().numpy() - a[4].cpu().numpy()) / np.abs(a[4].cpu().numpy())) < 2e-6
    # the y-pair copy (pair form: two 32-B pieces per cell, lane pairs)
    yp = ops.volume_ypair(vol)
    y = ops.local_phase(vol, *args, want_dvp=True, ypair=yp)
    assert np.max(np.abs(y[4].cpu().numpy() - a[4].cpu().numpy()) / np.abs(a[4].cpu().numpy())) < 2e-6
    # the device route, with and without the y-pair copy: the staged kernel
    # for compact clouds (>= half the sampled boxes fit), else the pair-form
    # y-pair kernel, or the box-less half-complex one without a copy
    for ypc in (yp, None):
        r = ops.local_phase(vol, *args, want_dvp=True, ypair=ypc, routed=True)
        want = 0 if spread < 5 else (2 if ypc is not None else 1)
        if spread != 8.0:     # 8 degrees sits near the 50 % threshold
            assert r[5] == want, (spread, frac, r[5])
        assert np.max(np.abs(r[4].cpu().numpy() - a[4].cpu().numpy()) / np.abs(a[4].cpu().numpy())) < 2e-6
    da, db = a[4].cpu().numpy(), b[4].cpu().numpy()
    assert np.max(np.abs(da - db) / np.abs(db)) < 2e-6      # pixel summation order only
    for l in range(nImg):
        *_, rd = orc.local_phase(s["vol"], s["vdim"], s["pf"], quat[l], trans[l], 1.0, pR[l],
                                 pT[l], s["dat"][l], s["ctf"][l], s["sig"][l], s["px"], s["N"])
        assert np.max(np.abs(da[l] - rd) / np.abs(rd)) < 1e-5


def test_resample_bit_exact(orc):
    rng = np.random.default_rng(5)
    for nIn, nOut, nImg in ((125, 125, 7), (2000, 125, 3), (151, 9, 4), (9, 9, 6)):
        w = rng.uniform(0.1, 1, (nImg, nIn))
        u = (rng.uniform(0, 1, (nImg, nIn)) ** 4).astype(np.float32)
        u0 = rng.uniform(0, 1.0 / nOut, nImg)
        anc, wo, imax = ops.resample(T(w), T(u), nOut, T(u0))
        anc, wo, imax = anc.cpu().numpy(), wo.cpu().numpy(), imax.cpu().numpy()
        for l in range(nImg):
            ra, rw, ri = orc.resample(w[l], u[l].astype(np.float64), nOut, u0[l])
            assert np.array_equal(anc[l], ra)
            assert np.array_equal(wo[l], rw)
            assert imax[l] == ri


@pytest.mark.parametrize("method,spread,mReco,dup", [
    ("direct", 0.0, 6, False), ("tiled", 0.0, 6, False), ("tiled", 2.0, 100, False),
    ("tiled", 8.0, 150, False), ("binned", 0.0, 6, False), ("binned", 2.0, 100, False),
    ("binned", 8.0, 150, False), ("binned", 2.0, 100, True), ("tiled", 2.0, 100, True)])
def test_insert3d(orc, stack, method, spread, mReco, dup):
    """spread 0: uniform samples (patch boxes overflow -> direct scatter;
    binned: entries spread over every tile); spread 2 deg: a posterior cloud,
    every patch accumulated in LDS; mReco 150 > 128: two sample tiles per
    image; dup: resampled-like samples, copies of 12 ancestors with their own
    translations (the binned insert merges each ancestor's copies)."""
    s = stack
    px = dev_pixels(s)
    nImg = 4
    rng = np.random.default_rng(21)
    if spread > 0:
        quat = synth.clustered_quaternions(nImg, mReco, spread, rng)
    else:
        quat = synth.uniform_quaternions(nImg * mReco, rng).reshape(nImg, mReco, 4)
    if dup:
        anc = rng.integers(0, 12, (nImg, mReco))
        quat = np.ascontiguousarray(np.take_along_axis(quat, anc[..., None], axis=1))
    trans = rng.standard_normal((nImg, mReco, 2)) * 3
    off = rng.standard_normal((nImg, 2))
    w = np.full(nImg, 1.0 / mReco, np.float32)
    hm = ops.HalfMap(s["vdim"], DEV)
    ops.insert3d(hm, T(s["dat"][:nImg]), T(s["ctf"][:nImg]), T(quat), T(trans), T(off), T(w), px,
                 method=method)
    F, Tm, O, cnt = orc.insert_batch(s["vdim"], s["pf"], s["dat"][:nImg], s["ctf"][:nImg], quat,
                                     trans, off, w, s["px"], s["N"])
    gF = hm.F.cpu().numpy().reshape(-1)
    gT = hm.T.cpu().numpy().reshape(-1)
    assert np.max(np.abs(gF - F)) <= 1e-5 * np.max(np.abs(F))
    assert np.max(np.abs(gT - Tm)) <= 1e-5 * np.max(np.abs(Tm))
    assert np.allclose(hm.O.cpu().numpy(), O, rtol=1e-12, atol=1e-12)
    assert int(hm.counter.item()) == cnt == nImg * mReco


@pytest.mark.parametrize("scale", [1e-6, 1e6])
def test_insert3d_binned_value_scale(orc, stack, scale):
    """The binned deposit accumulates in 64-bit fixed point scaled by the
    batch's largest |value|: data far from unit magnitude keep the 1e-5 bar."""
    s = stack
    px = dev_pixels(s)
    nImg, mReco = 4, 50
    rng = np.random.default_rng(5)
    quat = synth.clustered_quaternions(nImg, mReco, 3.0, rng)
    trans = rng.standard_normal((nImg, mReco, 2))
    off = np.zeros((nImg, 2))
    w = np.full(nImg, 1.0 / mReco, np.float32)
    dat = (s["dat"][:nImg] * scale).astype(np.complex64)
    hm = ops.HalfMap(s["vdim"], DEV)
    ops.insert3d(hm, T(dat), T(s["ctf"][:nImg]), T(quat), T(trans), T(off), T(w), px, method="binned")
    F, Tm, O, cnt = orc.insert_batch(s["vdim"], s["pf"], dat, s["ctf"][:nImg], quat, trans, off, w,
                                     s["px"], s["N"])
    gF = hm.F.cpu().numpy().reshape(-1)
    assert np.max(np.abs(gF - F)) <= 1e-5 * np.max(np.abs(F))
    assert np.max(np.abs(hm.T.cpu().numpy().reshape(-1) - Tm)) <= 1e-5 * np.max(np.abs(Tm))


def test_fsc(orc):
    vdim = 48
    rng = np.random.default_rng(7)
    shape = (vdim, vdim, vdim // 2 + 1)
    A = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    B = (A + 0.7 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)
    got = ops.fsc(T(A), T(B), vdim // 2).cpu().numpy()
    assert np.max(np.abs(got - orc.fsc(A, B, vdim, vdim // 2))) < 1e-6


def test_host_adapters_match_device_ops(orc, stack):
    """thx_Expect* / thx_InsertFT (Interface.h-shaped, host pointers)."""
    s = stack
    px = dev_pixels(s)
    L = lib()
    nR, nT, n = len(s["quat"]), len(s["trans"]), s["px"].n
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    traP = np.zeros((nT, n), np.complex64)
    mat = np.zeros((nR, 9))
    iCol, iRow = s["px"].iCol.copy(), s["px"].iRow.copy()
    q = np.ascontiguousarray(s["quat"])
    tr = np.ascontiguousarray(s["trans"])
    assert L.thx_ExpectRotran(P(traP), P(tr), P(q), P(mat), P(iCol), P(iRow), nR, nT, s["N"], n) == 0
    rotP = np.zeros((nR, n), np.complex64)
    vol = np.ascontiguousarray(s["vol"])
    assert L.thx_ExpectProject(P(vol), P(rotP), P(mat), P(iCol), P(iRow), nR, s["pf"], 1,
                               s["vdim"], n) == 0
    g_rot, g_tra = gpu_tables(orc, s, px)
    assert np.array_equal(rotP, g_rot.cpu().numpy())
    assert np.array_equal(traP, g_tra.cpu().numpy())
    nImg = len(s["dat"])
    pR = np.full(nR, 1.0 / nR)
    pT = np.full(nT, 1.0 / nT)
    wC = np.zeros(nImg, np.float32)
    wR = np.zeros(nImg * nR, np.float32)
    wT = np.zeros(nImg * nT, np.float32)
    base = np.zeros(nImg, np.float32)
    dat, ctf, sig = (np.ascontiguousarray(s[k]) for k in ("dat", "ctf", "sig"))
    assert L.thx_ExpectGlobal3D(P(rotP), P(traP), P(dat), P(ctf), P(sig), P(wC), P(wR), P(wT),
                                P(pR), P(pT), P(base), 0, 1, nR, nT, n, nImg) == 0
    ref = ops.global_scan(g_rot, g_tra, T(dat), T(ctf), T(sig), T(pR), T(pT), algo=4)
    assert np.array_equal(wR, ref[1].cpu().numpy().reshape(-1))
    assert np.array_equal(base, ref[3].cpu().numpy())
    # InsertFT
    mReco = 3
    rng = np.random.default_rng(2)
    iq = synth.uniform_quaternions(nImg * mReco, rng).reshape(nImg, mReco, 4)
    it = rng.standard_normal((nImg, mReco, 2))
    off = np.zeros((nImg, 2))
    w = np.full(nImg, 1.0 / mReco, np.float32)
    size = (s["vdim"] // 2 + 1) * s["vdim"] ** 2
    F = np.zeros(2 * size, np.float32)
    Tm = np.zeros(size, np.float32)
    O = np.zeros(3)
    cnt = np.zeros(1, np.int32)
    iColPad = (iCol * s["pf"]).astype(np.int32)
    iRowPad = (iRow * s["pf"]).astype(np.int32)
    assert L.thx_InsertFT(P(F), P(Tm), P(O), P(cnt), P(dat), P(ctf), P(off), P(w), P(iq), P(it),
                          P(iColPad), P(iRowPad), s["pf"], n, mReco, s["N"], s["vdim"], nImg) == 0
    rF, rT, rO, rc = orc.insert_batch(s["vdim"], s["pf"], dat, ctf, iq, it, off, w, s["px"], s["N"])
    assert np.max(np.abs(F - rF.view(np.float32))) <= 1e-5 * np.max(np.abs(rF.view(np.float32)))
    assert int(cnt[0]) == rc


@pytest.mark.parametrize("spread", [0.0, 2.0, 10.0, 40.0])
def test_particle_statistics_match_oracle(spread):
    """calVari (ACG spreads of the de-meaned cloud, translation sd),
    balanceWeight(PAR_R) priors and the peak factor / keepHalfHeightPeak of
    the device particle filter against oracle/particle.py (spread 0: the
    degenerate, all-equal cloud of a sharp reseed)."""
    from oracle import particle as op
    rng = np.random.default_rng(int(spread * 10) + 3)
    nImg, mR, mT = 6, 125, 9
    if spread > 0:
        quat = synth.clustered_quaternions(nImg, mR, spread, rng)
    else:
        quat = np.repeat(synth.uniform_quaternions(nImg, rng)[:, None, :], mR, axis=1)
    trans = rng.standard_normal((nImg, mT, 2)) * 2
    k, sd = ops.pf_calvari(T(quat), T(trans), 1e-4, 0.1)
    k, sd = k.cpu().numpy(), sd.cpu().numpy()
    for l in range(nImg):
        rk = np.maximum(1e-4, op.cal_vari_rot(quat[l]))
        assert np.allclose(k[l], rk, rtol=1e-6, atol=1e-12), (k[l], rk)
        assert np.allclose(sd[l], np.maximum(0.1, op.cal_vari_trans(trans[l])), rtol=1e-12)
    if spread > 0:
        pR = ops.pf_balance_rot(T(quat)).cpu().numpy()
        for l in range(nImg):
            assert np.allclose(pR[l], op.balance_rot(quat[l]), rtol=1e-6)
    u = rng.exponential(1.0, (nImg, 2000)).astype(np.float32) ** 4
    ud, peak = ops.pf_peak(T(u).clone())
    ud, peak = ud.cpu().numpy(), peak.cpu().numpy()
    for l in range(nImg):
        rp = op.peak_factor_rot(u[l])
        assert peak[l] == pytest.approx(rp, rel=1e-7)
        assert np.allclose(ud[l], op.keep_half_height(u[l], rp), rtol=1e-6, atol=1e-6 * u[l].max())


def _acg_iters(Q):
    """Iterations oracle/particle.py's infer_acg takes on cloud Q (the same loop, counted)."""
    B, it = np.eye(4), 0
    while True:
        it += 1
        A = B
        with np.errstate(all="ignore"):
            Ai = np.linalg.inv(A)
            u = np.einsum("ij,jk,ik->i", Q, Ai, Q)
            B = np.einsum("ij,ik->jk", Q / u[:, None], Q) * (4.0 / np.sum(1.0 / u))
        if not np.abs(A - B).sum() > 1e-3:
            return it


def test_calvari_replayed_second_fixed_point():
    """k_pf_calvari takes the de-meaned cloud's fixed point as the first
    one's iterates replayed through the de-meaning rotation
    (calvari_acg_impl), with the second pass's own stopping rule.  Against
    the oracle's two passes at 1e-6, on clouds where the oracle's second
    pass stops before, at and after its first (asserted: all three occur),
    resampled clouds of few ancestors, 200-particle clouds (the strided path)
    and clouds of 128 and 129 (the register path full, and one past it)."""
    from oracle import particle as op
    rng = np.random.default_rng(29)
    clouds = []
    for m in (125, 200):
        for spread in (1.0, 3.0, 10.0, 30.0, 60.0):
            clouds.append(synth.clustered_quaternions(6, m, spread, rng))
        clouds.append(np.stack([_runs_cloud(rng, 12, m, 3.0) for _ in range(6)]))
    # clouds whose de-meaned fixed point runs past the first (found by a
    # search over seeds): uniform clouds and a 40-degree cloud squeezed in x
    special = [synth.uniform_quaternions(125, np.random.default_rng(s)) for s in (1173, 1189)]
    for s in (1034, 1114):
        g = np.random.default_rng(s)
        q = synth.clustered_quaternions(1, 125, 40.0, g)[0]
        q[:, 1] *= 0.2
        special.append(q / np.linalg.norm(q, axis=1, keepdims=True))
    clouds.append(np.stack(special))
    # the register path exactly full (128 particles) and the strided path just
    # past it, from a generator of their own: the clouds above keep their draws
    rng_edge = np.random.default_rng(31)
    for m in (128, 129):
        for spread in (1.0, 3.0, 10.0, 30.0, 60.0):
            clouds.append(synth.clustered_quaternions(6, m, spread, rng_edge))
        clouds.append(np.stack([_runs_cloud(rng_edge, 12, m, 3.0) for _ in range(6)]))
    before = after = same = 0
    for quat in clouds:
        nImg, m = quat.shape[:2]
        trans = rng.standard_normal((nImg, 9, 2))
        k, _ = ops.pf_calvari(T(quat), T(trans), 0.0, 0.0)
        k = k.cpu().numpy()
        for l in range(nImg):
            mean = op.principal_axis(op.infer_acg(quat[l]))
            it1 = _acg_iters(quat[l])
            it2 = _acg_iters(op.qmul(op.conj(mean)[None, :], quat[l]))
            before += it2 < it1
            after += it2 > it1
            same += it2 == it1
            assert np.allclose(k[l], op.cal_vari_rot(quat[l]), rtol=1e-6, atol=1e-12), (m, l, it1, it2)
    assert before and after and same, (before, after, same)


@pytest.mark.parametrize("n", [9, 125, 2000, 2048, 2049, 5000])
def test_peak_factor_register_and_reread_paths(n):
    """k_pf_peak keeps rows of up to 2048 marginals in registers for its
    bisection and re-reads longer ones from memory: both paths, at and across
    the threshold, against oracle/particle.py -- random rows, rows of few
    distinct values (ties at the rank), constant rows and rows with zeros."""
    from oracle import particle as op
    rng = np.random.default_rng(n + 11)
    u = (rng.exponential(1.0, (4, n)) ** 4).astype(np.float32)
    u[1] = np.round(u[1] * 4) / 4 + 0.25            # ties
    u[2] = 0.75                                     # constant
    u[3, ::3] = 0.0                                 # zeros among the values
    ud, peak = ops.pf_peak(T(u).clone())
    ud, peak = ud.cpu().numpy(), peak.cpu().numpy()
    for l in range(4):
        rp = op.peak_factor_rot(u[l])
        assert peak[l] == pytest.approx(rp, rel=1e-7), (l, peak[l], rp)
        assert np.allclose(ud[l], op.keep_half_height(u[l], rp), rtol=1e-6, atol=1e-6 * u[l].max())


def _runs_cloud(rng, nAnc, m, spread):
    """A resampled cloud: nAnc ancestors drawn around one pose, their copies
    stored next to each other (as k_gather leaves them)."""
    anc = synth.clustered_quaternions(1, nAnc, spread, rng)[0]
    cnt = rng.multinomial(m - nAnc, np.full(nAnc, 1.0 / nAnc)) + 1
    return np.repeat(anc, cnt, axis=0)


@pytest.mark.parametrize("case", ["spread", "runs", "runs_capped", "large"])
def test_acg_mean_matches_oracle(case):
    """The driver's perturbation mean (k_pf_mean: inferACG capped at acgIters,
    then its principal axis) against oracle/particle.py on plain clouds,
    resampled clouds of 10 ancestors, 4-ancestor clouds, and 200-particle
    clouds (the strided, non-register path).  A 4-ancestor cloud that runs to
    the cap has no parity target: its A collapses towards rank 1 and the
    reference's own axis moves with the summation order (the oracle on a
    permuted cloud), so converged images are compared there at a looser
    tolerance and the capped ones must give a finite unit axis inside the
    cloud."""
    from oracle import particle as op
    rng = np.random.default_rng({"spread": 1, "runs": 2, "runs_capped": 3, "large": 4}[case])
    nImg, cap = 24, 100
    m = 200 if case == "large" else 125
    if case in ("spread", "large"):
        quat = synth.clustered_quaternions(nImg, m, 3.0, rng)
    else:
        nAnc = 10 if case == "runs" else 4
        sp = 3.0 if case == "runs" else 30.0
        quat = np.stack([_runs_cloud(rng, nAnc, m, sp) for _ in range(nImg)])
    mq = torch.empty(nImg, 4, dtype=torch.float64, device="cuda")
    it = torch.empty(nImg, dtype=torch.int32, device="cuda")
    dq = T(quat)
    assert lib().thx_pf_acg_mean(nImg, m, ops._ptr(dq), cap, ops._ptr(mq), ops._ptr(it), None) == 0
    torch.cuda.synchronize()
    mq, it = mq.cpu().numpy(), it.cpu().numpy()
    # 4-ancestor clouds converge slowly towards a near-singular A (tens of
    # iterations, stopping at sum|A - B| <= 1e-3, so a rounding difference can
    # move the stopping iteration): 1 - |cos| of the axis within 2e-3 there
    # (the oracle itself moves by 4e-4 on a permuted cloud), 1e-9 elsewhere;
    # the 10-ancestor case checks the run multiplicities at 1e-9
    tol = 2e-3 if case == "runs_capped" else 1e-9
    if case == "runs_capped":
        assert (it == cap).any(), it
    else:
        assert (it < cap).all(), it
    for l in range(nImg):
        if it[l] == cap:
            assert abs(np.linalg.norm(mq[l]) - 1.0) < 1e-12
            assert np.abs(quat[l] @ mq[l]).max() > 0.5
            continue
        ref = op.principal_axis(op.infer_acg(quat[l], cap))
        assert abs(abs(np.dot(mq[l], ref)) - 1.0) < tol, (l, it[l], mq[l], ref)


def test_empty_batches(orc, stack):
    """Zero images through every batch entry point: no launch, empty results
    (the reference loops over an empty image set)."""
    s = stack
    px = dev_pixels(s)
    rotP, traP = gpu_tables(orc, s, px)
    nR, nT = len(s["quat"]), len(s["trans"])
    e_dat = torch.empty(0, px.n, dtype=torch.complex64, device=DEV)
    e_f = torch.empty(0, px.n, dtype=torch.float32, device=DEV)
    for algo in (0, 1, 2, 4):
        wC, wR, wT, base = ops.global_scan(rotP, traP, e_dat, e_f, e_f,
                                           T(np.full(nR, 1.0 / nR)), T(np.full(nT, 1.0 / nT)),
                                           algo=algo)
        assert wR.shape == (0, 1, nR) and base.shape == (0,)
    q = torch.empty(0, 5, 4, dtype=torch.float64, device=DEV)
    t = torch.empty(0, 3, 2, dtype=torch.float64, device=DEV)
    one = lambda *sh: torch.ones(*sh, dtype=torch.float64, device=DEV)
    out = ops.local_phase(T(s["vol"]), q, t, one(0), one(0, 5), one(0, 3), e_dat, e_f, e_f, px,
                          want_dvp=True)
    assert out[4].shape == (0, 5, 3)
    k, sd = ops.pf_calvari(q, t)
    assert k.shape == (0, 3) and sd.shape == (0, 2)
    torch.cuda.synchronize()


def test_volume_ypair_layout():
    """thx_volume_ypair against the layout its header states: element
    (x, y, z) = (v(x, y, z), v(x, (y + 1) mod vdim, z)), the slices z, z+1
    of each even z interleaved: yp[z // 2, y, x, z % 2]."""
    vdim = 24
    g = torch.Generator().manual_seed(3)
    vol = torch.complex(torch.randn(vdim, vdim, vdim // 2 + 1, generator=g),
                        torch.randn(vdim, vdim, vdim // 2 + 1, generator=g)).to(DEV)
    yp = ops.volume_ypair(vol).cpu()
    v = vol.cpu()
    for zl in (0, 1):
        assert torch.equal(yp[:, :, :, zl, 0], v[zl::2])
        assert torch.equal(yp[:, :, :, zl, 1], torch.roll(v, -1, dims=1)[zl::2])

def _degenerate_clouds(rng, m=125):
    """Clouds whose ACG fixed point runs into (near-)singular matrices: two or
    three ancestors, all-but-one equal, and one pose stored as q and -q."""
    anc = lambda n: synth.clustered_quaternions(1, n, 3.0, rng)[0]
    out = [np.repeat(anc(2), [60, m - 60], axis=0),
           np.repeat(anc(3), [40, 40, m - 80], axis=0),
           np.repeat(anc(2), [m - 1, 1], axis=0)]
    q = np.repeat(anc(1), m, axis=0)
    q[::2] *= -1.0
    out.append(q)
    return np.stack(out)


def test_acg_degenerate_clouds():
    """inferACG on degenerate clouds, where the fixed point's reciprocals
    approach 0 or the normal-range limits (rcp_nr keeps the IEEE quotient
    there): calVari's spreads are finite and in [0, 1] (A(j, j) / A(0, 0) of
    the de-meaned cloud), the perturbation mean is a finite unit axis inside
    the cloud.  One pose stored as q and -q (the same rotation) has a
    well-defined answer, and the spreads match the oracle there at 1e-6.  On
    the rank-deficient clouds (two or three ancestors, all-but-one equal) the
    reference's fixed point runs towards a singular A: the oracle moves by up
    to 10x under a permutation of the cloud, and where the iteration stops
    depends on when a determinant or a quadratic form leaves the normal range
    (the all-but-one-equal cloud: 2e-6 in numpy's LU, exactly 0 here once the
    outlier's 1 / (q^T A^-1 q) is the IEEE 1 / inf), so there is no parity
    target (parity unpinned there): both sides must call the cloud collapsed
    (spreads <= 1e-2, against ~0.25 for a 30-degree cloud)."""
    from oracle import particle as op
    rng = np.random.default_rng(11)
    quat = _degenerate_clouds(rng)
    nImg, m = quat.shape[:2]
    trans = rng.standard_normal((nImg, 9, 2))
    k, _ = ops.pf_calvari(T(quat), T(trans), 0.0, 0.0)
    k = k.cpu().numpy()
    assert np.all(np.isfinite(k)) and np.all(k >= 0.0) and np.all(k <= 1.0), k
    for l in range(nImg):
        with np.errstate(all="ignore"):
            r = np.array(op.cal_vari_rot(quat[l]))
            p = np.array(op.cal_vari_rot(quat[l][rng.permutation(m)]))
        if l == nImg - 1:     # q / -q
            assert np.allclose(k[l], r, rtol=1e-6, atol=1e-12), (l, k[l], r)
        else:
            assert np.all(k[l] <= 1e-2) and np.all(r <= 1e-2) and np.all(p <= 1e-2), (l, k[l], r, p)
    mq = torch.empty(nImg, 4, dtype=torch.float64, device="cuda")
    it = torch.empty(nImg, dtype=torch.int32, device="cuda")
    assert lib().thx_pf_acg_mean(nImg, m, ops._ptr(T(quat)), 100, ops._ptr(mq), ops._ptr(it), None) == 0
    torch.cuda.synchronize()
    mq = mq.cpu().numpy()
    for l in range(nImg):
        assert np.all(np.isfinite(mq[l])) and abs(np.linalg.norm(mq[l]) - 1.0) < 1e-12, mq[l]
        assert np.abs(quat[l] @ mq[l]).max() > 0.5
