"""The between-round kernels (csrc/round.hip, thunder_amd/round.py) against
the float64 restatements of tests/round_ref.py, and one round end from the
expectation to the next local search.

thx_recentre's image is bounded like every other phase_shift output of the
project (the rule of test_gpu_subtract.py / test_gpu_noise.py): per image,
max |gpu - ref64| / max |ori_l| <= max(1e-5, 4 e32), e32 the same metric for
the restatement with the phase formed in FP32 against the float64 phase on
the same inputs -- what FP32 phase formation costs (the reference pays it
too); the factor covers the hardware sin / cos."""
import types

import numpy as np
import pytest
import torch

import round_ref
from thunder_amd import expectation as ex
from thunder_amd import ingest, noise, ops, synth
from thunder_amd import round as rnd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def T(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def unit(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


# ---------------------------------------------------------- thx_rank1st_diff
@pytest.mark.parametrize("nImg", [1, 255, 257])
def test_rank1st_diff(nImg):
    rng = np.random.default_rng(nImg)
    cur = {"quat": unit(rng, nImg), "trans": rng.standard_normal((nImg, 2)) * 0.5,
           "d": 1 + 0.05 * rng.standard_normal(nImg), "cls": rng.integers(0, 3, nImg).astype(np.int32)}
    prev = {"quat": unit(rng, nImg), "trans": rng.standard_normal((nImg, 2)) * 0.5,
            "d": 1 + 0.05 * rng.standard_normal(nImg), "cls": rng.integers(0, 3, nImg).astype(np.int32)}
    prev["quat"][0] = -cur["quat"][0]                       # the same rotation: diffR = 0
    ref, _ = round_ref.diff_top(cur, prev)
    order = ("cls", "quat", "trans", "d")
    r1 = tuple(T(cur[k]) for k in order)
    pv = tuple(T(prev[k]) for k in order)
    dR, dT, dD, sC = rnd.rank1st_change(r1, pv)
    for got, want in ((dR, ref["diffR"]), (dT, ref["diffT"]), (dD, ref["diffD"])):
        err = np.abs(got.cpu().numpy() - want).max()
        print("rank1st_diff max abs error", err)
        assert err <= 1e-15
    assert abs(float(dR[0])) <= 1e-15
    assert np.array_equal(sC.cpu().numpy(), ref["sameC"])
    for a, b in zip(r1, pv):                                # prev <- current, in place
        assert torch.equal(a, b)
    # NULL groups are skipped: only the translations, the rest untouched
    pv2 = tuple(T(prev[k]) for k in order)
    out = rnd.rank1st_change((None, None, r1[2], None), pv2)
    assert out[0] is None and out[2] is None and out[3] is None
    assert np.abs(out[1].cpu().numpy() - ref["diffT"]).max() <= 1e-15
    assert torch.equal(pv2[2], r1[2]) and torch.equal(pv2[1], T(prev["quat"]))
    assert torch.equal(pv2[0], T(prev["cls"])) and torch.equal(pv2[3], T(prev["d"]))


# ----------------------------------------------------------- thx_class_count
@pytest.mark.parametrize("nK", [1, 7, 64])
def test_class_count(nK):
    rng = np.random.default_rng(nK)
    a = rng.integers(-2, nK + 2, 1000).astype(np.int32)     # some outside [0, nK)
    b = rng.integers(0, nK, 257).astype(np.int32)
    count = rnd.class_count(T(a), nK)
    ref = round_ref.class_count(a, nK)
    assert np.array_equal(count.cpu().numpy(), ref)
    rnd.class_count(T(b), nK, count)                        # accumulates
    assert np.array_equal(count.cpu().numpy(), round_ref.class_count(b, nK, ref.copy()))
    distr = rnd.class_distribution(T(b), nK)
    assert np.allclose(distr.cpu().numpy(), np.bincount(b, minlength=nK) / 257.0, rtol=1e-15)
    with pytest.raises(ValueError):                         # nothing to normalise
        rnd.class_distribution(T(np.full(5, nK, np.int32)), nK)


# -------------------------------------------------------------- thx_recentre
def recentre_case(idim, nImg, mLT=9):
    """Updated offsets 0, integer, fractional, negative and beyond idim/2, by
    image in turn (the first a fractional one past idim/2)."""
    rng = np.random.default_rng(1000 * idim + nImg)
    h = idim / 2
    pat = np.array([[h + 1.3, -(h + 2.7)], [0.0, 0.0], [3.0, -2.0], [0.37, 1.61], [-4.25, -0.5]])
    new_off = pat[np.arange(nImg) % len(pat)]
    t = rng.standard_normal((nImg, 2)) * 2.0
    t[1::5] = 0.0                                           # with t = 0: offS = 0 exactly
    c = types.SimpleNamespace(idim=idim, n=nImg, t=t, off=new_off + t)
    c.ori = (rng.standard_normal((nImg, idim, idim // 2 + 1)) +
             1j * rng.standard_normal((nImg, idim, idim // 2 + 1))).astype(np.complex64)
    c.trans = rng.standard_normal((nImg, mLT, 2)) * 3.0
    c.prev = rng.standard_normal((nImg, 2))
    c.ref = round_ref.recentre(c.ori, c.t, c.off, c.trans, c.prev, fp32=False)
    c.ref32 = round_ref.recentre(c.ori, c.t, c.off, c.trans, c.prev, fp32=True)
    c.scale = np.abs(c.ori).reshape(nImg, -1).max(1)
    c.e32 = float((np.abs(c.ref32["img"] - c.ref["img"]).reshape(nImg, -1).max(1) / c.scale).max())
    return c


def image_error(c, img):
    return float((np.abs(img.cpu().numpy() - c.ref["img"]).reshape(c.n, -1).max(1) / c.scale).max())


@pytest.mark.parametrize("nImg", [1, 3, 130])
@pytest.mark.parametrize("idim", [8, 30, 64])
def test_recentre(idim, nImg):
    """Measured on an MI355X, by max |. - ref64| / max |ori_l|: the FP32-phase
    restatement e32 = 1.5e-6 .. 1.8e-6 at idim 8, 5.1e-6 .. 7.8e-6 at idim 30,
    6.8e-6 .. 1.79e-5 at idim 64 (the largest: idim 64, nImg 130, offsets past
    idim/2); the device 1.5e-6 .. 1.8e-6, 5.1e-6 .. 7.8e-6, 6.8e-6 .. 1.79e-5
    -- within 2 % of e32 in all nine cases, so the bound max(1e-5, 4 e32)
    leaves the hardware sin / cos a factor of about 4."""
    c = recentre_case(idim, nImg)
    ori, top, off, trans, prev = T(c.ori), T(c.t), T(c.off), T(c.trans), T(c.prev)
    img = torch.full_like(ori, float("nan"))
    rnd.recentre(ori, img, top, off, trans, prev)
    # the state: FP64 subtractions, exact
    assert np.array_equal(off.cpu().numpy(), c.ref["off"])
    assert np.array_equal(trans.cpu().numpy(), c.ref["trans"])
    assert np.array_equal(prev.cpu().numpy(), c.ref["prev_t"])
    assert (top == 0).all()
    assert torch.equal(ori, T(c.ori))
    err, bound = image_error(c, img), max(1e-5, 4 * c.e32)
    print(f"recentre idim {idim} nImg {nImg}: gpu {err:.3e} e32 {c.e32:.3e} bound {bound:.3e}")
    assert err <= bound
    # each optional part left out: the rest as before
    for drop in ("img", "trans", "prev"):
        top2, off2, trans2, prev2 = T(c.t), T(c.off), T(c.trans), T(c.prev)
        img2 = None if drop == "img" else torch.full_like(ori, float("nan"))
        rnd.recentre(ori, img2, top2, off2, None if drop == "trans" else trans2,
                     None if drop == "prev" else prev2)
        assert torch.equal(off2, off) and (top2 == 0).all()
        assert torch.equal(trans2, T(c.trans) if drop == "trans" else trans)
        assert torch.equal(prev2, T(c.prev) if drop == "prev" else prev)
        assert img2 is None or torch.equal(torch.view_as_real(img2), torch.view_as_real(img))


def test_recentre_with_remask_is_recentre_then_remask():
    c = recentre_case(32, 5)
    ori = T(c.ori)
    a, b = torch.empty_like(ori), torch.empty_like(ori)
    rnd.recentre(ori, a, T(c.t), T(c.off), remask=(11.0, 6.0))
    rnd.recentre(ori, b, T(c.t), T(c.off))
    ingest.remask(b, 11.0, 6.0)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    assert torch.isfinite(torch.view_as_real(a)).all()


# ------------------------------------------------------------ one round end
def test_round_end_smoke():
    """expectation -> rank1st -> noise update at that pose -> statistics ->
    re-centring -> a local search from the moved state, box 32: shapes,
    finiteness, and the local search still on the generating pose within the
    bounds of test_gpu_driver.py::test_local_search_refines_from_a_particle_state
    (median angle < 1.5 degrees, median shift error < 0.5 px)."""
    N, pf, n = 32, 2, 24
    vol = synth.projectee(synth.blob_volume(N, n_blobs=8, seed=7, device=DEV), pf)
    px = ops.PixelSet(N, pf, 14, 1, device=DEV)
    gset = synth.global_sample_set(400, seed=8)
    q, t = gset[0], gset[1]
    rng = np.random.default_rng(9)
    qtrue = T(q[rng.integers(0, len(q), n)])
    near = np.argsort(np.linalg.norm(t, axis=1))[:20]
    ttrue = T(t[near[rng.integers(0, len(near), n)]])
    attr = T(synth.ctf_attrs(n, seed=10))
    ctf = ops.ctf(attr, px)
    sigl = ctf * ops.project3d(vol, ops.rotmat(qtrue), px) * ops.trans_table(ttrue, px)
    dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=20.0, seed=11)
    # whole FT images holding the pixel set's data (zero elsewhere)
    iPxl = T(np.ascontiguousarray(px.iPxl, np.int64))
    ori = torch.zeros(n, N * (N // 2 + 1), dtype=torch.complex64, device=DEV)
    ori[:, iPxl] = dat
    ori = ori.reshape(n, N, N // 2 + 1).contiguous()
    img = ori.clone()
    offS = torch.zeros(n, 2, dtype=torch.float64, device=DEV)

    e = ex.Expectation(vol, px, gset, mLR=125, mLT=9, n_phase=4, seed=12)
    out = e.run(dat, ctf, sig)
    cls, quat, trans, d, vari = e.rank1st()
    assert quat.shape == (n, 4) and trans.shape == (n, 2) and vari.shape == (n, 6) and d is None
    assert torch.isfinite(quat).all() and torch.isfinite(trans).all() and torch.isfinite(vari).all()

    st = types.SimpleNamespace(N=N, imgFT=img, oriFT=ori, attr=attr, r_mask=0.35 * N)
    nm = noise.NoiseModel(N, 1, DEV)
    s2, rcp = nm.update(st, vol[None].contiguous(), quat, trans, pf, offS, None, cls)
    assert np.isfinite(s2).all() and np.isfinite(rcp).all()

    distr = rnd.class_distribution(cls, 1)
    assert distr.cpu().tolist() == [1.0]
    stats = rnd.refresh_variance(vari, two_d=False)
    assert all(np.isfinite(v).all() for v in stats.values())
    prev = (cls.clone(), quat.clone(), torch.zeros_like(trans), None)
    dR, dT, _, sC = rnd.rank1st_change((cls, quat, trans, None), prev)
    assert (dR.abs() <= 1e-15).all() and torch.allclose(dT, trans.norm(dim=1), rtol=1e-14, atol=0)
    assert rnd.refresh_rotation_change(dR)[0] <= 1e-15 and (sC == 1).all()

    t1 = trans.clone()
    cloud_t, prev_t = out[1], prev[2]
    rnd.recentre(ori, img, trans, offS, cloud_t, prev_t, remask=(0.35 * N, 6.0))
    # (rank1st_change left prev_t = t1, so it moves to 0 with the top itself)
    assert (trans == 0).all() and torch.equal(offS, -t1) and (prev_t == 0).all()
    assert torch.isfinite(torch.view_as_real(img)).all()

    dat2 = ingest.gather(img, px.iPxl)
    loc = ex.Expectation(vol, px, None, mLR=125, mLT=9, search="local", converge=True, seed=13)
    state = (out[0], cloud_t, out[2], out[3], cls)
    q2, t2, pR2, pT2, score2, cls2, nph2 = loc.run(dat2, ctf, sig, state=state)
    assert q2.shape == (n, 125, 4) and t2.shape == (n, 9, 2)
    assert torch.isfinite(q2).all() and torch.isfinite(t2).all() and torch.isfinite(score2).all()
    angle = lambda qq: torch.rad2deg(2 * torch.acos((qq * qtrue).sum(-1).abs().clamp(max=1)))
    ang = angle(ex.cloud_mode(q2))
    print("round end: median angle of the global search's top", float(angle(quat).median()))
    terr = (t2.mean(1) - (ttrue - t1)).norm(dim=-1)
    print("round end: median angle", float(ang.median()), "median shift error", float(terr.median()))
    assert float(ang.median()) < 1.5 and float(terr.median()) < 0.5
