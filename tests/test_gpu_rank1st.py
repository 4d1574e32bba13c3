"""The top particle the expectation driver exports (thx_expectation_rank1st,
Expectation.rank1st()): Particle::rank1st after the reseed, after a local
seed, under the stopping rule, in MODE_2D and with a CTF search -- and the
driver's seven outputs unchanged by it.  Box 32, pf 2, an asymmetric volume
(tests/stacks.py)."""
import ctypes

import numpy as np
import pytest
import torch

from stacks import small_stack
from thunder_amd import _lib, ops, synth
from thunder_amd import expectation as ex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, PF = 32, 2


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def device_stack(s):
    px = ops.PixelSet(s["N"], s["pf"], s["rU"], s["rL"], device=DEV)
    nR, nT = len(s["quat"]), len(s["trans"])
    gset = (s["quat"], s["trans"], np.full(nR, 1.0 / nR), np.full(nT, 1.0 / nT))
    return px, gset, T(s["dat"]), T(s["ctf"]), T(s["sig"])


def class_volumes(s, nK):
    """nK projectees: the stack's own and nK - 1 other blob volumes."""
    vols = [T(s["vol"])] + [synth.projectee(synth.blob_volume(N, n_blobs=8, seed=90 + k), PF).to(DEV)
                            for k in range(1, nK)]
    return torch.stack(vols).contiguous() if nK > 1 else vols[0]


def run_and_read(e, *args, **kw):
    """One run and its rank1st, read before anything else touches the scratch."""
    out = e.run(*args, **kw)
    r1 = e.rank1st()
    return [x.clone() for x in out], [None if x is None else x.clone() for x in r1]


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------ 1. scan only
@pytest.mark.parametrize("nK", [1, 3])
@pytest.mark.parametrize("nImg", [1, 5, 67])
def test_reseed_top_is_the_argmax_of_the_scan_marginals(orc, nImg, nK):
    """Global search without phases: topQuat / topTrans are, bit for bit, the
    global samples of largest marginal wR / wT in the drawn class (the
    marginals of thx_global_scan on the same inputs); vari holds the reseed's
    calVari."""
    s = small_stack(orc, N=N, nImg=nImg, nR=40, nT=12, seed=20 + nImg)
    px, gset, dat, ctf, sig = device_stack(s)
    vols = class_volumes(s, nK)
    e = ex.Expectation(vols, px, gset, mLR=16, mLT=9, n_phase=0, seed=3)
    out, (cls, quat, trans, d, vari) = run_and_read(e, dat, ctf, sig)
    assert d is None and torch.equal(cls, out[5])
    q, t, pR, pT = (T(x) for x in gset)
    traP = ops.trans_table(t, px)
    state = None
    for k in range(nK):
        vk = vols[k].contiguous() if nK > 1 else vols
        state = ops.global_scan(ops.project3d(vk, ops.rotmat(q), px), traP, dat, ctf, sig, pR, pT,
                                kIdx=k, nK=nK, state=state)
    _, wR, wT, _ = state
    idx = torch.arange(nImg, device=DEV)
    # the stack is one where the oracle's own marginals (float64, on the CPU)
    # have a unique maximum in the drawn class of every image
    ref = None
    for k in range(nK):
        vk = (vols[k] if nK > 1 else vols).cpu().numpy()
        dk = orc.dvp_global(vk, s["vdim"], s["pf"], s["quat"], s["trans"], s["dat"], s["ctf"],
                            s["sig"], s["px"], s["N"])
        ref = orc.weights_global(dk, gset[2], gset[3], kIdx=k, nK=nK, state=ref)
    c = cls.cpu().numpy()
    for r in (ref[1], ref[2]):
        row = np.asarray(r).reshape(nImg, nK, -1)[np.arange(nImg), c]
        top2 = np.sort(row, axis=1)[:, -2:]
        assert np.all(top2[:, 1] > top2[:, 0]), "the oracle's maximum must be unique"
    for w, grid, got in ((wR, q, quat), (wT, t, trans)):
        row = w[idx, cls.long()]                               # [nImg, n]
        top2 = row.topk(2, dim=1).values
        assert (top2[:, 0] > top2[:, 1]).all(), "the scan's maximum must be unique"
        assert torch.equal(got, grid[row.argmax(1)])
    assert torch.isfinite(vari).all() and (vari[:, :5] > 0).all() and (vari[:, 5] == 0).all()


# ------------------------------------------------------- local seed, no phase
def local_state(nImg, mR, mT, seed):
    rng = np.random.default_rng(seed)
    quat = synth.clustered_quaternions(nImg, mR, 3.0, rng)
    trans = rng.standard_normal((nImg, mT, 2))
    pR = rng.random((nImg, mR)) + 0.1
    pT = rng.random((nImg, mT)) + 0.1
    return (T(quat), T(trans), T(pR / pR.sum(1, keepdims=True)), T(pT / pT.sum(1, keepdims=True)))


@pytest.mark.parametrize("nImg", [1, 5, 257])
def test_local_seed_top_is_the_particle_of_largest_prior(orc, nImg):
    """A local search that runs no phase exports calRank1st of the caller's
    state: quat[argmax pR], trans[argmax pT]."""
    s = small_stack(orc, N=N, nImg=min(nImg, 5), nR=4, nT=4, seed=31)
    px, _, dat, ctf, sig = device_stack(s)
    rep = -(-nImg // dat.shape[0])
    dat, ctf, sig = (x.repeat(rep, 1)[:nImg].contiguous() for x in (dat, ctf, sig))
    st = local_state(nImg, 9, 9, 32)
    e = ex.Expectation(T(s["vol"]), px, None, mLR=9, mLT=9, n_phase=0, search="local", seed=3)
    _, (cls, quat, trans, d, vari) = run_and_read(e, dat, ctf, sig, state=tuple(x.clone() for x in st))
    idx = torch.arange(nImg, device=DEV)
    assert torch.equal(quat, st[0][idx, st[2].argmax(1)])
    assert torch.equal(trans, st[1][idx, st[3].argmax(1)])
    assert torch.isfinite(vari).all()


# ------------------------------------------------- 2. one phase, replayed
RNG_PERTURB, RNG_RESAMPLE_R, RNG_RESAMPLE_T = 2000, 3000, 4000   # csrc/optimiser.hip


def replay_phase(e, vol, px, dat, ctf, sig, st, mean, route):
    """Phase 0 of a local search with the one-launch entry points the driver
    is built from.  Returns the final clouds and priors, the perturbed
    (pre-resample) clouds, iMax of both resamplings and the phase's calVari.
    route: the kernel the driver's device route picked for the phase.  The
    likelihood is replayed through the same route (thx_local_phase_routed_ball,
    the driver's own entry): at 125 x 9 the route takes another kernel than
    plain thx_local_phase, whose marginals differ from it in the last bits --
    with thx_local_phase the replayed clouds still matched there and the first
    differing quantity was the resampled prior pR."""
    q, t, pR, pT = (x.clone() for x in st)
    n, mR = q.shape[:2]
    c = e.cfg
    k, sd = ops.pf_calvari(q, t)                            # local_seed
    if mean == "acg":
        m = torch.empty(n, 4, dtype=torch.float64, device=DEV)
        _lib.check(_lib.lib().thx_pf_acg_mean(n, mR, ops._ptr(q), c.acgIters, ops._ptr(m), None,
                                              ops._stream(DEV)), "thx_pf_acg_mean")
    else:
        m = ops.pf_top_by_weight(q, pR)
    # a local search's first phase perturbs by perturbFactorL
    ops.pf_perturb(q, t, m, k, sd, c.perturbFactorL, c.transS, c.transM, c.seed, RNG_PERTURB + 0,
                   pR=pR, pT=pT)
    pC = torch.ones(n, dtype=torch.float64, device=DEV)
    if route < 0:          # not routed: the plain phase
        _, wR, wT, _, _ = ops.local_phase(vol, q, t, pC, pR, pT, dat, ctf, sig, px)
    else:
        R = ops.ypair_ball_radius(px)
        _, wR, wT, _, _, got = ops.local_phase(vol, q, t, pC, pR, pT, dat, ctf, sig, px, routed=True,
                                               ball=ops.volume_ypair_ball(vol, R), ball_r=R)
        assert got == route, "the replay must run the kernel the driver ran"
    # keepHalfHeightPeak with the peak factor a fresh particle carries (PEAK_FACTOR_MIN)
    ops.pf_peak(wR, torch.full((n,), 1e-3, dtype=torch.float64, device=DEV))
    k1, sd1 = ops.pf_calvari(q, t)                          # of the pre-resample cloud
    ancR, pR1, iR, _, _ = ops.pf_resample(pR, wR, mR, c.seed, RNG_RESAMPLE_R + 0, bool(c.shuffle))
    ancT, pT1, iT, _, _ = ops.pf_resample(pT, wT, t.shape[1], c.seed, RNG_RESAMPLE_T + 0,
                                          bool(c.shuffle))
    q1 = ops.pf_gather(q, ancR, torch.empty_like(q), mR)
    t1 = ops.pf_gather(t, ancT, torch.empty_like(t), t.shape[1])
    return dict(out=(q1, t1, pR1, pT1), q=q, t=t, iR=iR.long(), iT=iT.long(), k=k1, sd=sd1)


@pytest.mark.parametrize("mean", ["acg", "top"])
@pytest.mark.parametrize("mR", [9, 125])
def test_one_phase_rank1st_is_the_perturbed_particle_of_largest_weight(orc, mR, mean):
    """A local search of one phase without the stopping rule, replayed launch
    by launch.  The replay first has to reproduce the driver's final clouds
    and priors bit for bit (that holds without the export too and guards the
    replay); then rank1st is the perturbed cloud at the resamplings' iMax and
    vari the calVari of that cloud."""
    s = small_stack(orc, N=N, nImg=5, nR=4, nT=4, seed=60)
    px, _, dat, ctf, sig = device_stack(s)
    vol = T(s["vol"])
    st = local_state(5, mR, 9, 61)
    e = ex.Expectation(vol, px, None, mLR=mR, mLT=9, n_phase=1, search="local", seed=9,
                       perturb_mean=mean)
    routes = e.track_routes(1)
    out, (cls, quat, trans, d, vari) = run_and_read(e, dat, ctf, sig,
                                                    state=tuple(x.clone() for x in st))
    r = replay_phase(e, vol, px, dat, ctf, sig, st, mean, int(routes[0]))
    for name, got, want in zip(("quat", "trans", "pR", "pT"), out[:4], r["out"]):
        assert torch.equal(got, want), f"the replay does not reproduce the driver's {name}"
    idx = torch.arange(5, device=DEV)
    assert torch.equal(quat, r["q"][idx, r["iR"]])
    assert torch.equal(trans, r["t"][idx, r["iT"]])
    assert torch.equal(vari[:, :3], r["k"]) and torch.equal(vari[:, 3:5], r["sd"])
    assert (vari[:, 5] == 0).all()
    # the export is the phase's, not the seed's: the perturbation moved the cloud
    assert not torch.equal(quat, st[0][idx, st[2].argmax(1)])


# ------------------------------------------------------- 3. stopping rule
@pytest.fixture(scope="module")
def mixed(orc):
    """30 images of mixed SNR (and a second, different stack of the same shape)."""
    def build(seed):
        parts = [small_stack(orc, N=N, nImg=15, nR=60, nT=12, seed=seed, snr=snr)
                 for snr in (0.05, 5.0)]
        s = parts[0]
        px, gset, *_ = device_stack(s)
        dat, ctf, sig = (T(np.concatenate([p[k] for p in parts])) for k in ("dat", "ctf", "sig"))
        return dict(vol=T(s["vol"]), px=px, gset=gset, dat=dat, ctf=ctf, sig=sig)
    return build(40), build(41)


def converge_run(m, data=None):
    d = data or m
    e = ex.Expectation(m["vol"], m["px"], m["gset"], mLR=64, mLT=9, seed=5, converge=True)
    return run_and_read(e, d["dat"], d["ctf"], d["sig"])


def test_stopping_rule_rank1st(mixed, monkeypatch):
    a, b = mixed
    out, r1 = converge_run(a)
    cls, quat, trans, d, vari = r1
    assert len(set(out[6].cpu().tolist())) >= 2, "the images must stop in different phases"
    assert torch.isfinite(quat).all() and torch.isfinite(trans).all() and torch.isfinite(vari).all()
    assert torch.allclose(quat.norm(dim=1), torch.ones(30, dtype=torch.float64, device=DEV),
                          rtol=0, atol=1e-12)
    # the same run again, and without the view order: the same top particles
    assert same(converge_run(a)[1], r1)
    monkeypatch.setenv("THX_VIEW_ORDER", "0")
    assert same(converge_run(a)[1], r1)
    monkeypatch.delenv("THX_VIEW_ORDER")
    # another stack on the same scratch, which still holds the first run's
    # values: every part of its rank1st is its own, not a stale copy -- equal
    # to that stack's rank1st on a cleared scratch, different from the first's
    ws = ops.workspace(1, DEV)
    other = converge_run(a, b)[1]
    assert ops.workspace(1, DEV).data_ptr() == ws.data_ptr()
    ws.zero_()
    fresh = converge_run(a, b)[1]
    assert ops.workspace(1, DEV).data_ptr() == ws.data_ptr()
    for k in (1, 2, 4):                        # quat, trans, vari
        assert torch.equal(other[k], fresh[k]) and not torch.equal(other[k], r1[k])


# ----------------------------------------------------- 4. 2D and CTF search
def test_2d_rows_and_ctf_search_top_defocus(orc):
    vdim = N * PF
    rng = np.random.default_rng(50)
    yy, xx = np.mgrid[:vdim, :vdim] - vdim // 2
    img = sum(rng.uniform(0.5, 1.5) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * w * w))
              for cx, cy, w in rng.uniform([-9, -9, 2], [9, 9, 4], (5, 3)))
    cl = T((np.fft.rfft2(np.fft.ifftshift(img)) / vdim).astype(np.complex64))
    px = ops.PixelSet(N, PF, 8, 1, device=DEV)
    n = 6
    th = rng.uniform(0, 2 * np.pi, n)
    ctf = ops.ctf(T(synth.ctf_attrs(n, seed=51)), px)
    sigl = ctf * ops.project2d(cl, T(np.stack([np.cos(th), np.sin(th)], 1)), px)
    dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=5.0, seed=52)
    gset = [t.cpu().numpy() for t in ops.global_sample_set2d(48, 12, 10.0, 53, DEV)]
    e = ex.Expectation(cl, px, gset, mLR=16, mLT=9, n_phase=2, seed=7, mode="2d")
    _, (cls, rot, trans, d, vari) = run_and_read(e, dat, ctf, sig)
    assert d is None and (rot[:, 2:] == 0).all() and torch.isfinite(trans).all()
    assert torch.allclose(rot[:, 0] ** 2 + rot[:, 1] ** 2, torch.ones(n, dtype=torch.float64, device=DEV),
                          rtol=0, atol=1e-12)
    assert torch.isfinite(vari).all() and (vari[:, 5] == 0).all()
    # topD without a CTF search is refused
    ws, nImg, _ = e._last
    buf = torch.empty(n, 4, dtype=torch.float64, device=DEV)
    st = _lib.lib().thx_expectation_rank1st(ctypes.byref(e.cfg), None, 1, n, px.n, 0, ops._ptr(ws),
                                            ws.numel(), ops._ptr(buf), ops._ptr(buf), ops._ptr(buf),
                                            None, ops._stream(DEV))
    assert st == 1 and b"topD" in _lib.lib().thx_last_error()

    # SEARCH_TYPE_CTF, 3D: the top defocus factor
    s = small_stack(orc, N=N, nImg=5, nR=4, nT=4, seed=54, snr=5.0)
    px3, _, dat3, _, sig3 = device_stack(s)
    st3 = local_state(5, 16, 9, 55)
    e3 = ex.Expectation(T(s["vol"]), px3, None, mLR=16, mLT=9, n_phase=2, search="ctf", seed=7, mLD=9)
    out = e3.run_ctf(dat3, T(synth.ctf_attrs(5, seed=55)), sig3, st3)
    cls, quat, trans, d, vari = e3.rank1st()
    assert d.shape == (5,) and torch.isfinite(d).all() and (d > 0).all()
    assert torch.isfinite(quat).all() and torch.isfinite(trans).all() and torch.isfinite(vari).all()
    assert (vari[:, 5] > 0).all() and torch.equal(cls, out[5])


# ------------------------------------------------------- 5. nothing moved
@pytest.mark.parametrize("mean", ["acg", "top"])
@pytest.mark.parametrize("mR", [9, 125])
def test_local_outputs_do_not_depend_on_the_reader(orc, mR, mean):
    s = small_stack(orc, N=N, nImg=5, nR=4, nT=4, seed=60)
    px, _, dat, ctf, sig = device_stack(s)
    st = local_state(5, mR, 9, 61)
    outs = []
    for read in (False, True):
        e = ex.Expectation(T(s["vol"]), px, None, mLR=mR, mLT=9, n_phase=1, search="local", seed=9,
                           perturb_mean=mean)
        out = e.run(dat, ctf, sig, state=tuple(x.clone() for x in st))
        if read:
            r1 = e.rank1st()
            assert all(torch.isfinite(x).all() for x in r1[1:] if x is not None)
        outs.append([x.clone() for x in out])
    assert len(outs[0]) == 7 and same(*outs)


def test_reader_is_capturable(orc):
    """thx_expectation_rank1st is copies on the stream and nothing else: it
    captures into a graph, and the replayed graph fills the same values."""
    s = small_stack(orc, N=N, nImg=5, nR=4, nT=4, seed=60)
    px, _, dat, ctf, sig = device_stack(s)
    e = ex.Expectation(T(s["vol"]), px, None, mLR=9, mLT=9, n_phase=1, search="local", seed=9)
    e.run(dat, ctf, sig, state=local_state(5, 9, 9, 61))
    want = [x.clone() for x in e.rank1st()[1:] if x is not None]
    ws, n, _ = e._last
    got = [torch.full_like(x, float("nan")) for x in want]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.lib().thx_expectation_rank1st(ctypes.byref(e.cfg), None, 0, n, px.n, len(px.order),
                                                ops._ptr(ws), ws.numel(), ops._ptr(got[0]),
                                                ops._ptr(got[1]), None, ops._ptr(got[2]),
                                                ops._stream(DEV))
    assert st == 0
    g.replay()
    torch.cuda.synchronize()
    assert same(got, want)


def test_converge_outputs_do_not_depend_on_the_reader(mixed):
    a, _ = mixed
    e = ex.Expectation(a["vol"], a["px"], a["gset"], mLR=64, mLT=9, seed=5, converge=True)
    plain = [x.clone() for x in e.run(a["dat"], a["ctf"], a["sig"])]
    assert len(plain) == 7 and same(plain, converge_run(a)[0])
