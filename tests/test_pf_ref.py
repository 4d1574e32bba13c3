"""The float64 restatement of the phase-to-phase kernels (tests/pf_ref.py)
stands on its own: its perturbation has the ACG's moments and the reference's
multiplication order, its reCentre and priors follow src/Particle.cpp, its
class draw has the frequencies of the cut marginals, and its stopping rule ends
hand-written sequences where src/Optimiser.cpp:1510-1615 ends them.  No GPU."""
import numpy as np
from scipy.integrate import quad

import pf_ref
import philox_ref
from oracle import particle as op


def unit(rng, *shape):
    q = rng.standard_normal(shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def acg_second_moments(lam):
    """E[x_a^2 / |x|^2] for x ~ N(0, diag(lam)): with 1 / |x|^2 = int_0^inf
    exp(-s |x|^2) ds the Gaussian integrates to
    int_0^inf lam_a / (1 + 2 lam_a s) prod_b (1 + 2 lam_b s)^(-1/2) ds."""
    lam = np.asarray(lam, np.float64)
    out = []
    for a in range(len(lam)):
        f = lambda s, a=a: lam[a] / (1 + 2 * lam[a] * s) / np.sqrt(np.prod(1 + 2 * lam * s))
        out.append(quad(f, 0, np.inf, epsabs=1e-13, epsrel=1e-12)[0])
    return np.array(out)


def test_perturbation_moments_are_the_acgs():
    """An all-equal cloud at the mean: conj(mean) r' are the draws d themselves."""
    rng = np.random.default_rng(1)
    nImg, mR = 256, 800                                  # 204800 draws
    kk = np.array([0.5, 0.05, 0.005])
    mean = unit(rng, nImg)
    quat = np.repeat(mean[:, None, :], mR, axis=1)
    out = pf_ref.perturb3d(quat, np.zeros((nImg, 1, 2)), mean, np.tile(kk, (nImg, 1)),
                           np.ones((nImg, 2)), 1.0, 10.0, 1e9, seed=11, stream_id=3)
    d = np.concatenate([op.qmul(np.tile(op.conj(mean[l]), (mR, 1)), out.quat[l])
                        for l in range(nImg)])
    assert len(d) >= 200000 and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-14)
    want = acg_second_moments(np.concatenate([[1.0], kk]))
    assert abs(want.sum() - 1.0) < 1e-10                 # the quadrature is normalised
    sq = d * d
    for a in (1, 2, 3):
        ratio = sq[:, a].mean() / sq[:, 0].mean()
        # delta method: var(A/B) ~ var(A - ratio B) / (n mean(B)^2)
        se = np.std(sq[:, a] - ratio * sq[:, 0], ddof=1) / np.sqrt(len(d)) / sq[:, 0].mean()
        assert abs(ratio - want[a] / want[0]) < 5 * se, (a, ratio, want[a] / want[0], se)
    # the three components are told apart by more than the bound
    assert want[1] / want[0] > 3 * want[2] / want[0] > 9 * want[3] / want[0]


def test_sandwich_order():
    rng = np.random.default_rng(2)
    nImg, mR = 3, 21
    quat, mean = unit(rng, nImg, mR), unit(rng, nImg)
    tr, sd = np.zeros((nImg, 2, 2)), np.ones((nImg, 2))
    # no spread (sd = 1e-30 beside a first component that is N(0, 1)): d = (+-1, 0, 0, 0)
    # to rounding and the cloud comes back up to sign
    out = pf_ref.perturb3d(quat, tr, mean, np.full((nImg, 3), 1e-60), sd, 1.0, 10.0, 1e9, 5, 0)
    err = np.minimum(np.abs(out.quat - quat).max(-1), np.abs(out.quat + quat).max(-1))
    assert err.max() < 1e-14
    # mean = identity: r' = d r, and not r d
    ident = np.tile([1.0, 0, 0, 0], (nImg, 1))
    k = np.tile([0.9, 0.4, 0.1], (nImg, 1))
    out = pf_ref.perturb3d(quat, tr, ident, k, sd, 2.0, 10.0, 1e9, 5, 0)
    d = pf_ref.rotation_draws(nImg, mR, 2.0 * np.sqrt(k), 5, 0)
    for l in range(nImg):
        assert np.abs(out.quat[l] - op.qmul(d[l], quat[l])).max() < 1e-15
        assert np.abs(out.quat[l] - op.qmul(quat[l], d[l])).max() > 1e-2
    # a general mean: conj(mean) r' = d conj(mean) r
    out = pf_ref.perturb3d(quat, tr, mean, k, sd, 2.0, 10.0, 1e9, 5, 0)
    for l in range(nImg):
        cm = np.tile(op.conj(mean[l]), (mR, 1))
        assert np.abs(op.qmul(cm, out.quat[l]) - op.qmul(d[l], op.qmul(cm, quat[l]))).max() < 1e-15


def test_rotation_draw_layout():
    """Particle i is draw i // 8 of lane i % 8; the sine branch follows the cosine."""
    d = pf_ref.rotation_draws(2, 19, np.ones((2, 3)), 9, 4)
    for l, i in ((0, 0), (1, 7), (1, 8), (0, 18)):
        w = 4 * (i // 8)
        u = [float(philox_ref.uniform(9, l, 4, i % 8, w + j)) for j in range(4)]
        x = np.array([np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]),
                      np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
                      np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]),
                      np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])])
        assert np.array_equal(d[l, i], x / np.linalg.norm(x))
    assert philox_ref.gauss2(9, 1, 4, 7, 0)[0] == philox_ref.gauss(9, 1, 4, 7)
    x = philox_ref._philox_4x32_10(9, 1, 4, 7, 5)
    assert philox_ref.word0(9, 1, 4, 7, 5) == x[0]


def test_recentre_and_translation_priors():
    rng = np.random.default_rng(3)
    nImg, mR, mT = 6, 11, 29
    transS, transM, pf = 1.5, 4.0, 0.5
    tr = rng.standard_normal((nImg, mT, 2)) * 5          # radius ~ 6: beyond transM
    sd = np.abs(rng.standard_normal((nImg, 2))) + 0.5
    quat, mean = unit(rng, nImg, mR), unit(rng, nImg)
    out = pf_ref.perturb3d(quat, tr, mean, np.ones((nImg, 3)), sd, pf, transS, transM, 21, 6)
    assert 0.3 < out.redrawn.mean() < 0.95
    rad = np.hypot(out.trans[..., 0], out.trans[..., 1])
    assert np.all(rad[~out.redrawn] <= transM)
    # lane by lane with a scalar counter: 4 draws per rotation the lane owns, then
    # 2 per translation and 2 more after each re-draw
    for l in range(nImg):
        for j in range(8):
            c = 4 * len(range(j, mR, 8))
            for i in range(j, mT, 8):
                gx, gy = philox_ref.gauss2(21, l, 6, j, c)
                c += 2
                x, y = tr[l, i, 0] + gx * sd[l, 0] * pf, tr[l, i, 1] + gy * sd[l, 1] * pf
                far = np.sqrt(x * x + y * y) > transM
                if far:
                    hx, hy = philox_ref.gauss2(21, l, 6, j, c)
                    c += 2
                    x, y = hx * transS, hy * transS
                assert out.redrawn[l, i] == far
                assert (out.trans[l, i, 0], out.trans[l, i, 1]) == (x, y), (l, i)
    # the re-drawn ones are N(0, transS): their second moment within five standard errors
    z = out.trans[out.redrawn].ravel() / transS
    assert abs(np.mean(z * z) - 1.0) < 5 * np.std(z * z, ddof=1) / np.sqrt(len(z))
    # priors: sum 1, and the reference's formula without floors on such a cloud
    assert np.allclose(out.pT.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    for l in range(nImg):
        t = out.trans[l]
        m, s = t.mean(axis=0), t.std(axis=0, ddof=1)
        pdf = np.exp(-(((t[:, 0] - m[0]) / s[0]) ** 2 + ((t[:, 1] - m[1]) / s[1]) ** 2) / 2) / \
            (2 * np.pi * s[0] * s[1])                    # gsl_ran_bivariate_gaussian_pdf, rho = 0
        w = 1.0 / pdf
        assert np.allclose(out.pT[l], w / w.sum(), rtol=1e-13, atol=0)
        assert np.array_equal(out.pT[l], pf_ref.balance_trans(t, floors=False))
    # the floors: a point cloud (a power of two of equal terms sums without
    # rounding, so 1 / mT comes out exactly) and a single particle
    assert np.array_equal(pf_ref.balance_trans(np.full((8, 2), 2.5)), np.full(8, 1 / 8))
    assert np.allclose(pf_ref.balance_trans(np.full((9, 2), 2.5)), 1 / 9, rtol=1e-15, atol=0)
    assert np.array_equal(pf_ref.balance_trans(np.array([[3.0, -1.0]])), [1.0])
    # one outlier among 2000: it sits sqrt(1999) sample sds out on both axes,
    # exp(-1999) underflows and the 1e-300 floor takes over
    far = np.zeros((2000, 2))
    far[0] = 1e3
    w = pf_ref.balance_trans(far)
    assert w[0] == 1.0 and np.all((w[1:] > 0) & (w[1:] < 1e-290))
    with np.errstate(all="ignore"):
        assert not np.isfinite(pf_ref.balance_trans(far, floors=False)).all()


def test_class_draw_frequencies():
    n = 1 << 15
    row = np.array([1.0, 0.995, 0.999, 0.5, 0.992, 0.1, 0.9905], np.float32)
    cls = pf_ref.class_draw(np.tile(row, (n, 1)), seed=7, stream_id=999)
    u = row.astype(np.float64)
    p = np.maximum(u - pf_ref.PEAK_FACTOR_C * u.max(), 0.0)
    p /= p.sum()
    freq = np.bincount(cls, minlength=len(row)) / n
    assert np.count_nonzero(p) == 5
    for c in range(len(row)):
        assert abs(freq[c] - p[c]) <= 5 * np.sqrt(p[c] * (1 - p[c]) / n), (c, freq[c], p[c])
    # one-hot rows return their class, wherever the shuffle put it
    for K in (1, 2, 7, 64):
        hot = np.arange(512) % K
        w = np.zeros((512, K), np.float32)
        w[np.arange(512), hot] = 0.25
        assert np.array_equal(pf_ref.class_draw(w, 3, 1), hot)
    # all equal: uniform
    K = 4
    cls = pf_ref.class_draw(np.full((n, K), 0.5, np.float32), 7, 0)
    freq = np.bincount(cls, minlength=K) / n
    assert np.all(np.abs(freq - 1 / K) <= 5 * np.sqrt((1 / K) * (1 - 1 / K) / n)), freq
    # the shuffle is a permutation that moves: the first entry of an all-zero
    # row's shuffled set is what the draw returns (cdf all zero)
    z = pf_ref.class_draw(np.zeros((n, K), np.float32), 7, 0)
    assert set(z.tolist()) == set(range(K))


def run_script(two_d, with_d, min_phase=2, last_phase=11):
    k, sd, dd, nP, nP_d = pf_ref.converge_script()
    st = pf_ref.converge_state(k.shape[1], with_d)
    for phase in range(k.shape[0]):
        pf_ref.converge_step(st, phase, min_phase, last_phase, k[phase], sd[phase],
                             dd[phase] if with_d else None, two_d)
    return st, (nP_d if with_d else nP)


def test_stopping_rule_hand_sequences():
    for two_d in (False, True):
        for with_d in (False, True):
            st, want = run_script(two_d, with_d)
            assert np.all(st["done"] == 1)
            assert np.array_equal(st["nP"], want), (two_d, with_d, st["nP"])
    st, _ = run_script(False, True)
    # the bests a finished image keeps are those of its last phase
    assert st["bestR"][0] == 1.0 and st["bestT"][0] == 1.0
    assert st["bestT"][3] == 0.95 and st["bestR"][3] == 2.0 and st["bestD"][9] == 0.95
    assert abs(st["bestR"][1] - 0.9 ** 6) < 1e-15
    # min_phase itself never stops ...
    k, sd, dd, _, _ = pf_ref.converge_script()
    st = pf_ref.converge_state(10)
    for phase in range(3):
        pf_ref.converge_step(st, phase, 2, 11, k[phase], sd[phase])
    assert not st["done"].any()
    # ... unless it is the last phase
    st = pf_ref.converge_state(10)
    for phase in range(3):
        pf_ref.converge_step(st, phase, 2, 2, k[phase], sd[phase])
    assert np.all(st["done"] == 1) and np.all(st["nP"] == 2)
    # a last phase before min_phase ends the loop without a check
    st = pf_ref.converge_state(10)
    pf_ref.converge_step(st, 0, 2, 0, k[0], sd[0])
    assert np.all(st["nP"] == 0) and np.all(st["bestR"] == pf_ref.DBL_MAX)


def test_compact():
    done = np.array([0, 1, 0, 0, 1, 0], np.int32)
    assert pf_ref.compact(6, done).tolist() == [0, 2, 3, 5]
    assert pf_ref.compact(6, done, [5, 4, 3, 2, 1, 0]).tolist() == [5, 3, 2, 0]
    assert pf_ref.compact(3).tolist() == [0, 1, 2]
