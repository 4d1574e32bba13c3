"""The kernels that turn one particle-filter phase of the 3D driver into the
next, each launched on its own (thx_pf_perturb, thx_pf_class, thx_pf_converge,
thx_pf_compact, thx_pf_gather, thx_pf_top_by_weight, thx_pf_top_copy) and
pinned against the float64 restatement tests/pf_ref.py, which
tests/test_pf_ref.py checks on its own.  The perturbation and the class draw
run on a counter RNG the restatement replays draw for draw, so they are
compared value by value, not by their statistics.

Bars: quaternions and translations 1e-12 absolute (tests/test_gpu_symmetry.py's
bar for particle counterparts; the translations are O(10)); the closed-form
translation priors 1e-9 relative (the 2D perturbation's bar); the rotation
priors, which pass through inferACG's fixed point, 1e-6 relative against
oracle.particle.balance_rot of the device's own cloud
(test_particle_statistics_match_oracle's bar); the stopping rule's bests 1e-15
relative (pow); everything else bit for bit."""
import numpy as np
import pytest
import torch

import pf_ref
from oracle import particle as op
from thunder_amd import ops
from thunder_amd._lib import check, lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K_CHOICES = np.array([1e-8, 0.3, 1.0, 2.5])      # both sides of PERTURB_K_MAX = 1
N_IMG = (1, 31, 32, 33)                          # 32 images a block, 8 a wave


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def unit(rng, *shape):
    q = rng.standard_normal(shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_state(seed, nImg, mR, mT, cloud=0.3):
    """Means uniform on the sphere, clouds around them (spread `cloud` in every
    direction: non-degenerate whatever the perturbation adds), translations
    O(10), a k per image from K_CHOICES (image 0: three distinct components)."""
    rng = np.random.default_rng(seed)
    mean = unit(rng, nImg)
    quat = mean[:, None, :] + cloud * rng.standard_normal((nImg, mR, 4))
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    trans = rng.standard_normal((nImg, mT, 2)) * 3
    k = K_CHOICES[rng.integers(0, 4, (nImg, 3))]
    k[0] = (2.5, 0.3, 1e-8)
    sd = rng.uniform(0.5, 2.0, (nImg, 2))
    return quat, trans, mean, k, sd


def device_perturb(n, quat, trans, mean, k, sd, pf, transS, transM, seed, sid, done=None,
                   sym=None, fill=None):
    """thx_pf_perturb on the first n images; numpy (quat, trans, pR, pT)."""
    dq, dt = T(quat[:n]), T(trans[:n])
    dm, dk, ds = T(mean[:n]), T(k[:n]), T(sd[:n])
    pR = pT = None
    if fill is not None:
        pR = torch.full(quat[:n].shape[:2], fill, dtype=torch.float64, device=DEV)
        pT = torch.full(trans[:n].shape[:2], fill, dtype=torch.float64, device=DEV)
    dd = None if done is None else T(np.asarray(done[:n], np.int32))
    pR, pT = ops.pf_perturb(dq, dt, dm, dk, ds, pf, transS, transM, seed, sid, done=dd, symQ=sym,
                            pR=pR, pT=pT)
    torch.cuda.synchronize()
    return dq.cpu().numpy(), dt.cpu().numpy(), pR.cpu().numpy(), pT.cpu().numpy()


def compare(got, ref, n, check_pR):
    """Device (quat, trans, pR, pT) of n images against the restatement's
    first n; returns the largest deviations (quat, trans, pT rel, pR rel)."""
    q, t, pR, pT = got
    eq = np.abs(q - ref.quat[:n]).max()
    et = np.abs(t - ref.trans[:n]).max()
    ep = (np.abs(pT - ref.pT[:n]) / ref.pT[:n]).max()
    er = 0.0
    if check_pR:
        for l in range(n):
            want = op.balance_rot(q[l])
            er = max(er, (np.abs(pR[l] - want) / want).max())
    print(f"perturb n={n} mR={q.shape[1]} mT={t.shape[1]}: quat {eq:.3g} trans {et:.3g} "
          f"pT rel {ep:.3g} pR rel {er:.3g}")
    assert eq < 1e-12 and et < 1e-12, (eq, et)
    assert ep < 1e-9, ep
    assert er < 1e-6, er
    if check_pR:
        assert np.allclose(pR.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    return eq, et, ep, er


@pytest.mark.parametrize("pf", [0.5, 5.0])
@pytest.mark.parametrize("mR, mT", [(1, 1), (7, 2), (8, 9), (9, 9), (125, 9), (1000, 151)])
def test_perturb_matches_restatement(mR, mT, pf):
    """Image l's result depends on its own row and (seed, l, stream_id) only,
    so one restatement of 33 images serves every batch size."""
    seed, sid = 1234 + mR, 40 + mT
    st = make_state(100 + mR, max(N_IMG), mR, mT)
    ref = pf_ref.perturb3d(*st, pf, 10.0, 1e9, seed, sid)
    assert not ref.redrawn.any()
    for n in N_IMG:
        got = device_perturb(n, *st, pf, 10.0, 1e9, seed, sid)
        # rotation priors: on non-degenerate clouds only (Tyler's fixed point
        # wants many more particles than dimensions)
        compare(got, ref, n, check_pR=mR >= 125)


@pytest.mark.parametrize("mR, mT", [(9, 9), (8, 151), (125, 30)])
def test_recentre(mR, mT):
    """Translations beyond transM are re-drawn at width transS, which moves the
    lane's counter for every particle after them."""
    nImg, pf, transS, transM = 33, 1.0, 2.0, 6.0
    seed, sid = 77, 5
    st = make_state(7 + mT, nImg, mR, mT)
    ref = pf_ref.perturb3d(*st, pf, transS, transM, seed, sid)
    share = ref.redrawn.mean()
    assert 0.02 < share < 0.5, share
    # the guard: no decision within rounding of a tie
    assert ref.guard_t.min() > 1e-9, ref.guard_t.min()
    # every lane with more than one particle has re-draws ahead of later particles
    if mT > 8:
        assert ref.redrawn[:, :mT - 8].any()
    for n in (1, 33):
        got = device_perturb(n, *st, pf, transS, transM, seed, sid)
        compare(got, ref, n, check_pR=False)
        rad = np.hypot(got[1][..., 0], got[1][..., 1])
        assert np.all(rad[~ref.redrawn[:n]] <= transM)


@pytest.mark.parametrize("mT", [1, 8, 9, 16])
def test_translation_prior_floor(mT):
    """An all-equal translation set with sd = 0 stays all equal; its sample sd
    is 0, the 1e-6 floor applies and the priors are uniform -- exactly 1 / mT
    where mT is a power of two (sums of equal terms are then exact), within a
    few ulp otherwise."""
    nImg, mR = 9, 8
    quat, trans, mean, k, sd = make_state(3, nImg, mR, mT)
    trans[:] = (2.5, -1.25)
    sd[:] = 0.0
    ref = pf_ref.perturb3d(quat, trans, mean, k, sd, 1.0, 10.0, 20.0, 5, 1)
    _, t, _, pT = device_perturb(nImg, quat, trans, mean, k, sd, 1.0, 10.0, 20.0, 5, 1)
    assert np.array_equal(t, trans)
    if mT & (mT - 1) == 0:
        assert np.array_equal(pT, np.full((nImg, mT), 1.0 / mT))
    assert np.abs(pT * mT - 1.0).max() <= 1e-15
    assert (np.abs(pT - ref.pT) / ref.pT).max() < 1e-9


def test_translation_prior_pdf_floor():
    """One outlier among 2000 equal translations lies sqrt(1999) sample sds out
    on both axes: its pdf underflows, the 1e-300 floor applies before the
    inverse, and the priors stay finite and normalised."""
    nImg, mR, mT = 2, 8, 2000
    quat, trans, mean, k, sd = make_state(4, nImg, mR, mT)
    trans[:] = 0.0
    trans[0, 0] = trans[1, mT - 1] = 1e3
    sd[:] = 0.0
    ref = pf_ref.perturb3d(quat, trans, mean, k, sd, 1.0, 10.0, 1e9, 5, 1)
    _, t, _, pT = device_perturb(nImg, quat, trans, mean, k, sd, 1.0, 10.0, 1e9, 5, 1)
    assert np.array_equal(t, trans)
    assert pT[0, 0] == 1.0 and pT[1, mT - 1] == 1.0
    assert np.all(pT > 0) and (pT < 1e-290).sum() == nImg * (mT - 1)
    assert (np.abs(pT - ref.pT) / ref.pT).max() < 1e-9


@pytest.mark.parametrize("name", ["C4", "D2"])
@pytest.mark.parametrize("mR", [9, 125])
def test_perturb_symmetry_counterpart(name, mR):
    """symmetrise(&mean): every perturbed rotation is replaced by the group
    copy nearest the perturbation mean."""
    nImg, mT, pf = 33, 9, 5.0                     # pf 5: the cloud covers the sphere
    seed, sid = 31, 2
    _, symQ = ops.symmetry(name)
    assert len(symQ) == 3
    st = make_state(11 + mR, nImg, mR, mT)
    ref = pf_ref.perturb3d(*st, pf, 10.0, 1e9, seed, sid, sym=symQ)
    plain = pf_ref.perturb3d(*st, pf, 10.0, 1e9, seed, sid)
    moved = np.abs(ref.quat - plain.quat).max(axis=-1) > 1e-3
    assert 0.2 < moved.mean() < 0.98              # the counterpart is mostly another copy
    assert ref.guard_sym.min() > 1e-9, ref.guard_sym.min()
    mean = st[2]
    for n in (1, 33):
        q, t, pR, pT = got = device_perturb(n, *st, pf, 10.0, 1e9, seed, sid, sym=symQ)
        compare(got, ref, n, check_pR=False)
        # on its own: no group copy of an output is nearer the mean than the output
        for l in range(n):
            own = np.abs(q[l] @ mean[l])
            for sq in symQ:
                cp = op.qmul(np.tile(op.conj(sq), (mR, 1)), q[l])
                assert np.all(np.abs(cp @ mean[l]) < own)


def test_perturb_done_mask_and_streams():
    nImg, mR, mT, pf = 33, 9, 9, 1.0
    st = make_state(21, nImg, mR, mT)
    quat, trans = st[0], st[1]
    args = (pf, 2.0, 6.0, 99, 8)
    done = np.zeros(nImg, np.int32)
    done[[0, 12, 32]] = 1                          # first, mid-wave, last
    sentinel = -7.0
    free = device_perturb(nImg, *st, *args, fill=sentinel)
    mask = device_perturb(nImg, *st, *args, done=done, fill=sentinel)
    on = done == 1
    assert np.array_equal(mask[0][on], quat[on]) and np.array_equal(mask[1][on], trans[on])
    assert np.all(mask[2][on] == sentinel) and np.all(mask[3][on] == sentinel)
    for a, b in zip(mask, free):
        assert np.array_equal(a[~on], b[~on])
        assert np.all(b != sentinel)
    again = device_perturb(nImg, *st, *args, fill=sentinel)
    for a, b in zip(again, free):
        assert np.array_equal(a, b)
    other = device_perturb(nImg, *st, pf, 2.0, 6.0, 99, 9, fill=sentinel)
    assert np.all(np.abs(other[0] - free[0]).max(axis=(1, 2)) > 1e-6)
    assert np.all(np.abs(other[1] - free[1]).max(axis=(1, 2)) > 1e-6)
    # an all-zero mask is no mask
    none = device_perturb(nImg, *st, *args, done=np.zeros(nImg, np.int32), fill=sentinel)
    for a, b in zip(none, free):
        assert np.array_equal(a, b)


def test_perturb2d_translation_half():
    """perturb_trans behind thx_pf_perturb2d with a finite transM.  The 2D
    rotation draws take a data-dependent number of uniforms, so the stream is
    not replayed: the priors are checked in closed form on the device's own
    translations, and reCentre by its invariant."""
    nImg, mR, mT, pf, transS, transM = 33, 16, 30, 1.0, 1.0, 6.0
    rng = np.random.default_rng(4)
    th = rng.uniform(0, 2 * np.pi, (nImg, mR))
    rot = np.stack([np.cos(th), np.sin(th), 0 * th, 0 * th], -1)
    trans = rng.standard_normal((nImg, mT, 2)) * 3
    k, sd = np.full((nImg, 3), 0.05), rng.uniform(0.5, 2.0, (nImg, 2))

    def run(tm):
        dR, dT, dk, ds = T(rot), T(trans), T(k), T(sd)
        pR = torch.empty(nImg, mR, dtype=torch.float64, device=DEV)
        pT = torch.empty(nImg, mT, dtype=torch.float64, device=DEV)
        check(lib().thx_pf_perturb2d(nImg, mR, mT, ops._ptr(dR), ops._ptr(dT), ops._ptr(pR),
                                     ops._ptr(pT), ops._ptr(dk), ops._ptr(ds), pf, transS, tm, 17,
                                     3, None), "thx_pf_perturb2d")
        torch.cuda.synchronize()
        return dR.cpu().numpy(), dT.cpu().numpy(), pT.cpu().numpy()

    r0, t0, p0 = run(1e9)
    r1, t1, p1 = run(transM)
    assert np.array_equal(r0, r1)
    rad0 = np.hypot(t0[..., 0], t0[..., 1])
    assert 0.02 < (rad0 > transM).mean() < 0.5
    # a fresh N(0, 1) draw lies beyond 6 with probability e^-18: all are inside
    assert np.all(np.hypot(t1[..., 0], t1[..., 1]) <= transM)
    # a lane's first translation starts from the same counter in both runs: kept
    # bit for bit when within transM, replaced when beyond
    first = rad0[:, :8] <= transM
    assert np.array_equal(t1[:, :8][first], t0[:, :8][first])
    assert np.all(np.any(t1[:, :8][~first] != t0[:, :8][~first], axis=-1))
    for t, p in ((t0, p0), (t1, p1)):
        for l in range(nImg):
            want = pf_ref.balance_trans(t[l])
            assert (np.abs(p[l] - want) / want).max() < 1e-9


def class_rows(rng, nImg, K):
    """Row l % 5: random, one-hot, ties at the maximum, all equal, all zero."""
    w = rng.random((nImg, K), dtype=np.float32)
    for l in range(nImg):
        kind = l % 5
        if kind == 1:
            w[l] = 0
            w[l, rng.integers(K)] = 0.75
        elif kind == 2:
            w[l, rng.integers(0, K, 3)] = 1.5
        elif kind == 3:
            w[l] = 0.125
        elif kind == 4:
            w[l] = 0
    return w


@pytest.mark.parametrize("nImg", [1, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 2, 4, 7, 64])
def test_class_draw_bit_exact(K, nImg):
    rng = np.random.default_rng(K * 1000 + nImg)
    w = class_rows(rng, nImg, K)
    dw = T(w)
    cls = ops.pf_class(dw, 2024, 999).cpu().numpy()
    assert np.array_equal(cls, pf_ref.class_draw(w, 2024, 999))
    hot = np.arange(nImg) % 5 == 1
    assert np.array_equal(cls[hot], w[hot].argmax(axis=1))
    if nImg >= 255 and K >= 4:
        assert not np.array_equal(cls, ops.pf_class(dw, 2024, 998).cpu().numpy())


@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("two_d", [False, True])
def test_converge_scripted_phases(two_d, with_d):
    """Twelve phases of the hand-written script, tiled past one block; the
    device state is compared after every phase.  The bests start from a value
    that would deny room if the first check did not count from min_phase."""
    k, sd, dd, nP, nP_d = pf_ref.converge_script()
    reps = 26                                      # 260 images: two blocks
    k, sd, dd = np.tile(k, (1, reps, 1)), np.tile(sd, (1, reps, 1)), np.tile(dd, (1, reps))
    want_nP = np.tile(nP_d if with_d else nP, reps)
    n = k.shape[1]
    st = pf_ref.converge_state(n, with_d)
    for name in ("bestR", "bestT", "bestD"):
        if name in st:
            st[name][:] = 1e-9
    st["nP"][:] = -1
    dev = {name: T(v) for name, v in st.items()}
    for phase in range(k.shape[0]):
        dk, ds, dD = T(k[phase]), T(sd[phase]), T(dd[phase])
        prev = {name: v.cpu().numpy() for name, v in dev.items()}
        ops.pf_converge(phase, 2, 11, dk, ds, dev["bestR"], dev["bestT"], dev["done"], dev["nP"],
                        sdD=dD if with_d else None, bestD=dev.get("bestD"), two_d=two_d)
        was = st["done"] == 1                      # done before this phase
        pf_ref.converge_step(st, phase, 2, 11, k[phase], sd[phase], dd[phase] if with_d else None,
                             two_d)
        for name, v in st.items():
            got = dev[name].cpu().numpy()
            if v.dtype == np.int32:
                assert np.array_equal(got, v), (phase, name)
            else:
                assert np.all(np.abs(got - v) <= 1e-15 * np.abs(v)), (phase, name)
            # images that were done before this phase are not rewritten
            assert np.array_equal(got[was], prev[name][was]), (phase, name)
    assert np.all(st["done"] == 1) and np.array_equal(st["nP"], want_nP)
    assert np.array_equal(dev["nP"].cpu().numpy(), want_nP)


@pytest.mark.parametrize("nImg", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000])
def test_compact(nImg):
    rng = np.random.default_rng(nImg)
    perm = rng.permutation(nImg).astype(np.int32)
    masks = {"none": None, "zeros": np.zeros(nImg, np.int32), "all": np.ones(nImg, np.int32),
             "random": (rng.random(nImg) < 0.3).astype(np.int32)}
    for mname, done in masks.items():
        for order in (None, perm):
            dd = None if done is None else T(done)
            do = None if order is None else T(order)
            act, nAct = ops.pf_compact(nImg, DEV, done=dd, order=do)
            act, nAct = act.cpu().numpy(), int(nAct.cpu()[0])
            want = pf_ref.compact(nImg, done, order)
            assert nAct == len(want), (mname, order is not None)
            assert np.array_equal(act[:nAct], want), (mname, order is not None)
            assert np.all(act[nAct:] == -1)


@pytest.mark.parametrize("width", [1, 2, 4])
@pytest.mark.parametrize("shared", [True, False])
def test_gather(width, shared):
    rng = np.random.default_rng(width)
    sentinel = -3.0
    # the last shape is past one pass of the kernel's 1024 x 256 grid-stride loop
    for nImg, nOut, nIn in ((37, 11, 23), (37, 11, 11), (1100, 250, 250)):
        src = rng.standard_normal((nIn, width) if shared else (nImg, nIn, width))
        anc = rng.integers(0, nIn, (nImg, nOut)).astype(np.int32)
        done = (rng.random(nImg) < 0.3).astype(np.int32)
        done[[0, nImg - 1]] = 1
        want = src[anc] if shared else src[np.arange(nImg)[:, None], anc]
        dsrc, danc, ddone = T(src), T(anc), T(done)
        on = done == 1
        modes = [(None, False), (ddone, False)]
        if not shared and nIn == nOut:
            modes.append((ddone, True))
        for dmask, keep in modes:
            dst = torch.full((nImg, nOut, width), sentinel, dtype=torch.float64, device=DEV)
            ops.pf_gather(dsrc, danc, dst, nIn, done=dmask, keep_done=keep)
            got = dst.cpu().numpy()
            if dmask is None:
                assert np.array_equal(got, want)
                continue
            assert np.array_equal(got[~on], want[~on])
            if keep:
                assert np.array_equal(got[on], src[on])
            else:
                assert np.all(got[on] == sentinel)
    assert nImg * nOut * width > 1024 * 256


@pytest.mark.parametrize("nImg", [1, 256, 257])
def test_top_by_weight_and_top_copy(nImg):
    rng = np.random.default_rng(nImg)
    mR = 9
    quat = unit(rng, nImg, mR)
    pR = rng.random((nImg, mR))
    pR[1::7] = 0.25                                # all equal: particle 0
    pR[::3, 6] = pR[::3, 3] = 2.0                  # ties at the maximum: the first wins
    dq, dp = T(quat), T(pR)
    top = ops.pf_top_by_weight(dq, dp).cpu().numpy()
    best = pR.argmax(axis=1)                       # numpy's argmax is first-wins too
    flat = np.arange(nImg) % 7 == 1
    flat &= np.arange(nImg) % 3 != 0
    assert np.all(best[::3] == 3) and np.all(best[flat] == 0)
    assert np.array_equal(top, quat[np.arange(nImg), best])
    # k_top_copy: per-image and shared sources, with a done mask
    idx = rng.integers(0, mR, nImg).astype(np.int32)
    done = (rng.random(nImg) < 0.3).astype(np.int32)
    di, dd = T(idx), T(done)
    shared = unit(rng, mR)
    dsh = T(shared)
    for src, dsrc, want in ((quat, dq, quat[np.arange(nImg), idx]), (shared, dsh, shared[idx])):
        for dmask in (None, dd):
            out = torch.full((nImg, 4), -3.0, dtype=torch.float64, device=DEV)
            got = ops.pf_top_copy(dsrc, di, out, done=dmask).cpu().numpy()
            on = done == 1 if dmask is not None else np.zeros(nImg, bool)
            assert np.array_equal(got[~on], want[~on]) and np.all(got[on] == -3.0)
