"""thx_pf_load (Particle::load for a whole batch, csrc/load.hip) and
thx_pf_score against the float64 restatement tests/load_ref.py, which replays
the kernel's counter RNG draw for draw, and one table -> particle state ->
local search -> table round trip through thunder_amd/table.py.

Bars, those of tests/test_gpu_pf_phase.py for the same family: quaternions,
translations and defocus factors 1e-12 absolute; the closed-form priors pT /
pD 1e-9 relative; the rotation priors, which pass through inferACG's fixed
point, 1e-6 relative against oracle.particle.balance_rot of the device's own
cloud where that file compares them (mR >= 125), their sums 1 within 1e-12;
vari bit for bit what thx_pf_calvari / thx_pf_defocus(vari) give on the
returned clouds; thx_pf_score 1e-14 relative (pow); a saved column within
5e-10 of the device value (%18.9f).

Where the rotation priors are compared with the oracle.  thx_pf_load's pR is
by contract what thx_pf_balance_rot returns on the cloud, and that is asserted
bit for bit on every image.  That kernel inverts inferACG's 4x4 scatter matrix
by its adjugate in plain FP64: with the matrix's eigenvalues l1 >= l2 >= l3 >=
l4 (those of diag(1, k1, k2, k3) up to the sample's noise), an adjugate entry
along the two tightest directions is l1 l3 l4, summed from terms of size l1 (l1
l2) that each carry eps of relative rounding, so its relative error is about
eps l1^2 / (l3 l4).  The oracle inverts by LU and does not lose those digits.
The 1e-6 bar is therefore asserted where that estimate is a tenth of it,
eps l1^2 / (l3 l4) <= 1e-7 (for a tight cloud: the product of its two smallest k
at least 2.2e-9), and the largest deviation elsewhere is printed.  Measured on an
MI355X, 257 images with k from 5e-7 to 5: inside that domain at most 3.5e-8 at
(125, 9, 1) and 4.7e-7 at (1000, 151, 9); outside it 25 images beyond 1e-6 at
either shape, the worst 7.4e-3 at k = (1.0e-6, 1.2e-6, 5.7e-7) -- such a table row (a score near 1000) gets priors of three
digits from the driver's kernel, here as in every phase of a search."""
import os
import types

import numpy as np
import pytest
import torch

import load_ref
import pf_ref
from oracle import particle as op
from thunder_amd import expectation as ex
from thunder_amd import ingest, io, ops, synth, table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N_IMG = (1, 5, 33, 257)                  # a partial wave, a block of 32 images and one more, 9 blocks
SHAPES = [(1, 1, 0), (7, 2, 1), (8, 9, 1), (9, 9, 3), (125, 9, 1), (1000, 151, 9)]
# k as a table holds it: its score column is compressR = (k1 k2 k3)^(-1/6), so
# k = 1e-6 (a rotation known to 0.1 degrees, score 1000) .. 2.5 (beyond
# PERTURB_K_MAX: a cloud over the whole sphere, score 0.6)
K_MAGNITUDES = np.array([1e-6, 1e-5, 1e-4, 1e-3, 3e-2, 0.3, 1.0, 2.5])
SEED, SID = 4321, 6


def T(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def make_rows(seed, n):
    """Table rows: poses uniform on the sphere, every k component from
    K_MAGNITUDES with a jitter (image 0: three distinct components), shifts of
    a few pixels, spreads of O(1) pixel and O(1 %) defocus."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    k = K_MAGNITUDES[rng.integers(0, len(K_MAGNITUDES), (n, 3))] * rng.uniform(0.5, 2.0, (n, 3))
    k[0] = (2.5, 0.3, 1e-8)
    return {"q": q, "k": k, "t": rng.standard_normal((n, 2)) * 3, "sd": rng.uniform(0.5, 2.0, (n, 2)),
            "d": 1 + 0.05 * rng.standard_normal(n), "sdD": rng.uniform(1e-3, 2e-2, n)}


def device_load(rows, n, mR, mT, mD, seed=SEED, sid=SID, want_vari=True):
    """thx_pf_load on the first n rows -> device (quat, trans, pR, pT, d, pD, vari)."""
    out = table.pf_load(T(rows["q"][:n]), T(rows["k"][:n]), T(rows["t"][:n]), T(rows["sd"][:n]),
                        mR, mT, T(rows["d"][:n]) if mD else None, T(rows["sdD"][:n]) if mD else None,
                        mD, seed, sid, want_vari=want_vari)
    torch.cuda.synchronize()
    return out


_cases = {}


def case(shape):
    """The rows of a shape, their restatement at the largest batch and the
    device's result there: made once, read by every test, never modified."""
    if shape not in _cases:
        mR, mT, mD = shape
        n = max(N_IMG)
        rows = make_rows(100 + mR, n)
        ref = load_ref.load(rows["q"], rows["k"], rows["t"], rows["sd"], rows["d"], rows["sdD"],
                            mR, mT, mD, SEED, SID)
        _cases[shape] = (rows, ref, device_load(rows, n, mR, mT, mD))
    return _cases[shape]


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    """Bit for bit (NaN included: a degenerate cloud's statistics)."""
    return (a is None and b is None) or torch.equal(bits(a), bits(b))


def resolvable(k):
    """eps l1^2 / (l3 l4) <= 1e-7 over the eigenvalues of diag(1, k1, k2, k3):
    the clouds whose rotation priors plain FP64 resolves to a tenth of the bar
    (see the module's docstring)."""
    lam = np.sort(np.concatenate([np.ones((len(k), 1)), k], axis=1), axis=1)
    return np.finfo(np.float64).eps * lam[:, 3] ** 2 / (lam[:, 0] * lam[:, 1]) <= 1e-7


def rel(got, want):
    return float((np.abs(got - want) / np.abs(want)).max()) if want.size else 0.0


# ------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_load_matches_restatement(shape):
    mR, mT, mD = shape
    rows, ref, big = case(shape)
    n = max(N_IMG)
    quat, trans, pR, pT, d, pD, vari = big
    q, t = quat.cpu().numpy(), trans.cpu().numpy()
    eq, et = np.abs(q - ref.quat).max(), np.abs(t - ref.trans).max()
    ep = rel(pT.cpu().numpy(), ref.pT)
    ed = epd = 0.0
    if mD:
        ed = np.abs(d.cpu().numpy() - ref.d).max()
        epd = rel(pD.cpu().numpy(), ref.pD)
    else:
        assert d is None and pD is None
    er = er_out = 0.0
    if mR >= 125:
        r = pR.cpu().numpy()
        inside = resolvable(rows["k"])
        assert 0.3 * n < inside.sum() < n
        for l in range(n):
            e = rel(r[l], op.balance_rot(q[l]))
            er, er_out = (max(er, e), er_out) if inside[l] else (er, max(er_out, e))
        assert np.allclose(r.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    print(f"load {shape}: quat {eq:.3g} trans {et:.3g} d {ed:.3g} pT rel {ep:.3g} pD rel {epd:.3g} "
          f"pR rel {er:.3g} (clouds FP64 does not resolve: {er_out:.3g})")
    assert eq < 1e-12 and et < 1e-12 and ed < 1e-12, (eq, et, ed)
    assert ep < 1e-9 and epd < 1e-9, (ep, epd)
    assert er < 1e-6, er

    # vari: the driver's own statistics on the returned clouds, bit for bit
    k, sd = ops.pf_calvari(quat, trans)
    assert same(vari[:, 0:3], k) and same(vari[:, 3:5], sd)
    sdD = torch.zeros(n, dtype=torch.float64, device=DEV)
    if mD:
        ops.pf_defocus("vari", d, sd=sdD)
    assert same(vari[:, 5], sdD)
    assert same(pR, ops.pf_balance_rot(quat))
    # ... and the closed-form ones against gsl_stats_sd in numpy (sums of <= 151
    # terms of O(1) in float64: the priors' 1e-9 bar is loose for them)
    v = vari.cpu().numpy()
    if mT > 1:
        assert rel(v[:, 3:5], ref.trans.std(axis=1, ddof=1)) < 1e-9
    else:
        assert np.all(v[:, 3:5] == 0)
    if mD > 1:
        assert rel(v[:, 5], ref.d.std(axis=1, ddof=1)) < 1e-9
    else:
        assert np.all(v[:, 5] == 0)
    if mR >= 125:
        want = np.array([load_ref.stats(q[l], t[l], ref.d[l])[1][:3] for l in range(3)])
        print(f"load {shape}: k against oracle.cal_vari_rot, rel {rel(v[:3, :3], want):.3g}")

    # ---- 3. image l depends on its own row and (seed, l, stream_id) only
    for m in N_IMG[:-1]:
        small = device_load(rows, m, mR, mT, mD)
        for a, b in zip(small, big):
            assert same(a, None if b is None else b[:m]), m
    again = device_load(rows, n, mR, mT, mD)
    assert all(same(a, b) for a, b in zip(again, big))
    # without vari: the same clouds and priors
    bare = device_load(rows, n, mR, mT, mD, want_vari=False)
    assert bare[6] is None and all(same(a, b) for a, b in zip(bare[:6], big[:6]))


def test_another_stream_draws_another_cloud():
    shape = (9, 9, 3)
    rows, _, big = case(shape)
    other = device_load(rows, max(N_IMG), *shape, sid=SID + 1)
    seeded = device_load(rows, max(N_IMG), *shape, seed=SEED + 1)
    for alt in (other, seeded):
        for a, b in zip(alt[:6], big[:6]):
            # every image moved, not just some
            assert (a != b).reshape(a.shape[0], -1).any(dim=1).all()


# ------------------------------------------------ 2. product order and sign
@pytest.mark.parametrize("shape", [(9, 9, 3), (125, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_perturbation_on_the_left_with_the_drawn_sign(shape):
    """quat_i conj(q) = (p_i s_i q) conj(q) = s_i p_i.  Were the product taken
    the other way round (q p), it is conj(q) quat_i that would give s_i p_i:
    on image 0, whose k has three distinct components, that is far off."""
    rows, ref, big = case(shape)
    q = big[0].cpu().numpy()
    n, mR = q.shape[:2]
    assert (ref.sign == 1).any() and (ref.sign == -1).any()
    worst = 0.0
    for l in range(n):
        cq = np.tile(op.conj(rows["q"][l]), (mR, 1))
        worst = max(worst, np.abs(op.qmul(q[l], cq) - ref.sign[l][:, None] * ref.pert[l]).max())
    print(f"load {shape}: quat conj(q) against +-pert {worst:.3g}")
    assert worst < 1e-12
    cq = np.tile(op.conj(rows["q"][0]), (mR, 1))
    wrong = np.abs(op.qmul(cq, q[0]) - ref.sign[0][:, None] * ref.pert[0]).max()
    print(f"load {shape}: the right-hand form on image 0 is off by {wrong:.3g}")
    assert wrong > 1e-3
    # the k are not capped at PERTURB_K_MAX = 1: image 0's k1 = 2.5 is used as given
    assert rows["k"][0, 0] > 1
    capped = pf_ref.rotation_draws(1, mR, np.sqrt(np.minimum(1.0, rows["k"][:1])), SEED, SID)
    assert np.abs(capped[0] - ref.pert[0]).max() > 1e-3


# ---------------------------------------------------------------- 4. floors
@pytest.mark.parametrize("mT, mD", [(1, 1), (8, 8), (9, 3), (16, 9)])
def test_zero_spreads_keep_the_top_values(mT, mD):
    """sd = 0: every translation is topTrans exactly, the sample sd is 0, the
    1e-6 floor applies and pT is uniform (test_translation_prior_floor's bar);
    sdD = 0 likewise through balanceWeight(PAR_D)'s s == 0 branch."""
    n, mR = 9, 8
    rows = make_rows(3, n)
    rows["sd"][:] = 0.0
    rows["sdD"][:] = 0.0
    quat, trans, pR, pT, d, pD, vari = device_load(rows, n, mR, mT, mD)
    assert np.array_equal(trans.cpu().numpy(), np.repeat(rows["t"][:, None, :], mT, axis=1))
    assert np.array_equal(d.cpu().numpy(), np.repeat(rows["d"][:, None], mD, axis=1))
    pT, pD = pT.cpu().numpy(), pD.cpu().numpy()
    if mT & (mT - 1) == 0:
        assert np.array_equal(pT, np.full((n, mT), 1.0 / mT))
    assert np.abs(pT * mT - 1.0).max() <= 1e-15
    assert np.abs(pD * mD - 1.0).max() <= 1e-15
    # (the mean of equal values need not be that value to the last bit)
    assert np.all(vari[:, 3:6].cpu().numpy() <= 1e-14)


def test_no_defocus_samples():
    """mD == 0 with NULL defocus pointers.  A lane's sign uniforms follow its
    defocus draws, and the one defocus factor of mD = 1 is lane 0's: without it
    lane 0's rotations (i = 0 mod 8) keep their values up to the sign, every
    other rotation is unchanged, and so are the translations and everything
    that is even in the rotations (pR, vari)."""
    rows, _, big = case((125, 9, 1))
    out = device_load(rows, 33, 125, 9, 0)
    assert out[4] is None and out[5] is None
    lane0 = torch.arange(125, device=DEV) % 8 == 0
    assert same(out[0][:, ~lane0], big[0][:33][:, ~lane0])
    assert same(out[0].abs(), big[0][:33].abs())
    flipped = (out[0][:, lane0] != big[0][:33][:, lane0]).any(dim=-1).double().mean()
    assert 0.3 < float(flipped) < 0.7
    for j in (1, 2, 3):
        assert same(out[j], big[j][:33])
    assert same(out[6][:, :5], big[6][:33, :5]) and (out[6][:, 5] == 0).all()


# ---------------------------------------------------------- 5. thx_pf_score
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_score(n):
    rng = np.random.default_rng(n)
    vari = np.concatenate([10.0 ** rng.uniform(-12, 1, (n, 3)), rng.uniform(0, 3, (n, 3))], axis=1)
    vari[0, :3] = (1e-12, 1e-12, 1e-12)
    vari[-1, :3] = (10.0, 10.0, 10.0)
    s3 = table.pf_score(T(vari)).cpu().numpy()
    s2 = table.pf_score(T(vari), two_d=True).cpu().numpy()
    e3 = rel(s3, (vari[:, 0] * vari[:, 1] * vari[:, 2]) ** (-1.0 / 6))
    e2 = rel(s2, 1.0 / vari[:, 0])
    print(f"score n={n}: 3D rel {e3:.3g} 2D rel {e2:.3g}")
    assert e3 < 1e-14 and e2 < 1e-14
    w = table.grading_weights(T(vari), 4).cpu().numpy()
    assert w.dtype == np.float32 and np.array_equal(w, (s3 / 4).astype(np.float32))
    flat = table.grading_weights(T(vari), 4, grade=False).cpu().numpy()
    assert np.array_equal(flat, np.full(n, 0.25, np.float32))


# ------------------------------------------- 6. through a file, end to end
def geodesic_deg(a, b):
    return np.degrees(2 * np.arccos(np.minimum(1.0, np.abs((a * b).sum(-1)))))


def test_table_to_local_search_to_table(tmp_path):
    """32 images of a blob volume (box 64, pf 2, SNR 20) at known poses; a
    table holding those poses turned by 4 degrees about random axes and
    shifted by one pixel, k1 = k2 = k3 = sin^2(2 deg), stdTrans = 1; loaded,
    re-centred, searched locally for 5 phases and saved again.  The search
    must end nearer the truth than the table it started from.

    The pixel set ends at radius 14: a table 4 degrees (0.07 rad) off is worth
    searching to the radius where that error moves a pixel by one pixel, 1 /
    0.07 = 14, which is how a refinement sets its cutoff from the accuracy it
    has.  (At radius 28 the likelihood's peak is about 2 degrees wide and 125
    particles spread over 4 degrees per axis put one particle inside it on
    average: measured on an MI355X, the median error was then 8.8 degrees
    after one phase, 5.5 after five and 4.2 after ten -- and bit for bit the
    same from the tests/load_ref.py state uploaded in the loader's place, so a
    property of the search at that resolution, not of the loader.)  Measured
    at radius 14: 4.000 degrees in the table, 0.574 after the search; the
    shift error 1.000 -> 0.072 pixel."""
    N, pf, n = 64, 2, 32
    rng = np.random.default_rng(17)
    vol = synth.projectee(synth.blob_volume(N, n_blobs=12, seed=7, device=DEV), pf)
    px = ops.PixelSet(N, pf, 14, 1, device=DEV)
    qtrue = rng.standard_normal((n, 4))
    qtrue /= np.linalg.norm(qtrue, axis=1, keepdims=True)
    ttrue = rng.standard_normal((n, 2)) * 1.5
    attr = T(synth.ctf_attrs(n, seed=10))
    ctf = ops.ctf(attr, px)
    sigl = ctf * ops.project3d(vol, ops.rotmat(T(qtrue)), px) * ops.trans_table(T(ttrue), px)
    dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=20.0, seed=11)
    iPxl = T(np.ascontiguousarray(px.iPxl, np.int64))
    ori = torch.zeros(n, N * (N // 2 + 1), dtype=torch.complex64, device=DEV)
    ori[:, iPxl] = dat
    ori = ori.reshape(n, N, N // 2 + 1).contiguous()
    stack = types.SimpleNamespace(N=N, oriFT=ori, imgFT=ori.clone(), attr=attr)

    # the table: 4 degrees and one pixel off
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    turn = np.concatenate([np.full((n, 1), np.cos(np.radians(2.0))),
                           np.sin(np.radians(2.0)) * axis], axis=1)
    qtab = op.qmul(turn, qtrue)
    ang = rng.uniform(0, 2 * np.pi, n)
    ttab = ttrue + np.stack([np.cos(ang), np.sin(ang)], axis=1)
    t0 = io.thu_table(n, [f"{i + 1:06d}@stack.mrcs" for i in range(n)], quat=qtab, trans=ttab)
    t0["k1"][:] = t0["k2"][:] = t0["k3"][:] = np.sin(np.radians(2.0)) ** 2
    t0["stdTransX"][:] = t0["stdTransY"][:] = 1.0
    first = str(tmp_path / "start.thu")
    io.write_thu(first, t0)
    t1 = io.read_thu(first)
    before = geodesic_deg(np.stack([t1[f"quat{j}"] for j in range(4)], axis=1), qtrue)
    assert abs(np.median(before) - 4.0) < 1e-6

    loaded = table.particles_from_table(t1, mLR=125, mLT=9, seed=21, device=DEV)
    assert all(torch.isfinite(x).all() for x in loaded.state[:4]) and torch.isfinite(loaded.vari).all()
    assert torch.equal(loaded.score, T(t1["score"]))
    offS = table.start_local_search(stack, loaded)
    assert np.array_equal(offS.cpu().numpy(), -np.stack([t1["transX"], t1["transY"]], axis=1))
    assert (loaded.top[1] == 0).all()
    dat2 = ingest.gather(stack.imgFT, px.iPxl)

    e = ex.Expectation(vol, px, None, mLR=125, mLT=9, n_phase=5, search="local", seed=13)
    out = e.run(dat2, ctf, sig, state=loaded.state)
    cls, quat, trans, d, vari = e.rank1st()
    assert d is None and torch.equal(cls, T(t1["classID"].astype(np.int32)))
    for x in (quat, trans, vari, out[4]):
        assert torch.isfinite(x).all()
    t2 = table.round_table(t1, cls, quat, trans, d, vari, offS)
    path = table.save_database(str(tmp_path) + os.sep, t2, it=1)
    got = io.read_thu(path)

    score = table.pf_score(vari)
    want = {"classID": cls, "k1": vari[:, 0], "k2": vari[:, 1], "k3": vari[:, 2],
            "transX": trans[:, 0] - offS[:, 0], "transY": trans[:, 1] - offS[:, 1],
            "stdTransX": vari[:, 3], "stdTransY": vari[:, 4], "stdDefocusFactor": vari[:, 5],
            "score": score}
    for j in range(4):
        want[f"quat{j}"] = quat[:, j]
    for name in io.THU_COLUMNS:
        if name in io._THU_STR:
            assert got[name] == t1[name]
            continue
        w = want[name].double().cpu().numpy() if name in want else np.asarray(t1[name], np.float64)
        err = np.abs(np.asarray(got[name], np.float64) - w).max()
        assert err <= 5e-10, (name, err)

    after = geodesic_deg(np.stack([got[f"quat{j}"] for j in range(4)], axis=1), qtrue)
    terr = np.linalg.norm(np.stack([got["transX"], got["transY"]], axis=1) - ttrue, axis=1)
    print(f"table round trip: median geodesic error {np.median(before):.3f} deg in the table, "
          f"{np.median(after):.3f} deg after the search; median shift error 1.000 px -> "
          f"{np.median(terr):.3f} px")
    assert np.median(after) < np.median(before)
