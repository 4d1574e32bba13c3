"""CPU-side checks of post-processing (csrc/postprocess.hip,
thunder_amd/postprocess.py, tests/postprocess_ref.py): every new entry point
rejects bad arguments before any device work and the workspace queries are
host-only; known answers for the numpy restatement; its two shell-index forms
agree; the bound the GPU tests use separates four real mistakes; the FSC file's
line format and run()'s size check."""
import ctypes

import numpy as np
import pytest

import postprocess_cases as pc
import postprocess_ref as ref
from thunder_amd import _lib, build, io

OK, BAD = 0, 1
d = ctypes.c_void_p(4096)
d2 = ctypes.c_void_p(1 << 40)
BIG = ctypes.c_size_t(1 << 40)
NAN, INF = float("nan"), float("inf")
BAD_N = (31, 33, 14, 0, -2, 1026, 2048)         # odd, out of [16, 1024]


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def test_merge_weight_validates_without_gpu(L):
    call = lambda N=32, A=d, B=d2, fsc=d, nShell=15, dst=d: L.thx_ft_merge_weight(A, B, N, fsc, nShell,
                                                                                  dst, None)
    for N in BAD_N:
        assert call(N=N, nShell=5) == BAD, N
    assert b"N=" in L.thx_last_error()
    for ns in (0, 1, 17, -3):
        assert call(nShell=ns) == BAD
    assert b"nShell" in L.thx_last_error()
    assert call(A=None) == BAD and call(dst=None) == BAD
    assert b"NULL" in L.thx_last_error()


def test_bfactor_est_validates_without_gpu(L):
    call = lambda N=32, F=d, rL=3, rU=11, out=d, ws=d, n=BIG: L.thx_bfactor_est(
        F, N, rL, rU, None, None, out, None, ws, n, None)
    for N in BAD_N:
        assert call(N=N, rU=5) == BAD, N
    assert b"N=" in L.thx_last_error()
    for rU in (0, -1, 17, 4000):
        assert call(rU=rU) == BAD
    assert b"rU" in L.thx_last_error()
    assert call(rL=-1) == BAD
    assert b"rL" in L.thx_last_error()
    assert call(F=None) == BAD and call(out=None) == BAD
    need = L.thx_bfactor_est_workspace(32, 11)
    assert need > 0
    assert call(n=ctypes.c_size_t(need - 1)) == BAD
    assert b"workspace" in L.thx_last_error()
    assert call(ws=None) == BAD


def test_sharpen_validates_without_gpu(L):
    call = lambda N=32, src=d, b=-50.0, bDev=None, thres=0.3, tDev=None, ew=0.1, dst=d: \
        L.thx_ft_sharpen(src, N, b, bDev, thres, tDev, ew, dst, None)
    for N in BAD_N:
        assert call(N=N) == BAD, N
    assert b"N=" in L.thx_last_error()
    assert call(b=NAN) == BAD and call(b=INF) == BAD
    assert b"bFactor" in L.thx_last_error()
    assert call(thres=NAN) == BAD and call(thres=-INF) == BAD
    assert b"thres" in L.thx_last_error()
    assert call(ew=NAN) == BAD and call(ew=INF) == BAD
    assert b"ew" in L.thx_last_error()
    assert call(src=None) == BAD and call(dst=None) == BAD


def test_postprocess_validates_without_gpu(L):
    def call(N=32, nShell=15, A=d, B=d2, alpha=d, px=1.0, low=10.0, edge=4.0, bIn=NAN, method=0,
             fsc=d, info=d, fit=d, sharp=d, avg=None, ws=d, n=BIG):
        return L.thx_postprocess(A, B, N, nShell, alpha, px, low, edge, bIn, 1, method, fsc, None,
                                 info, fit, None, avg, sharp, ws, n, None)
    for N in BAD_N:
        assert call(N=N, nShell=5) == BAD, N
    assert b"N=" in L.thx_last_error()
    for ns in (0, 1, 17, -3):
        assert call(nShell=ns) == BAD
    assert b"nShell" in L.thx_last_error()
    assert call(method=3) == BAD and call(method=-1) == BAD
    assert call(N=48, nShell=23, method=2) == BAD
    for v in (NAN, INF, 0.0, -1.0):
        assert call(px=v) == BAD
    assert b"pixelSize" in L.thx_last_error()
    for v in (NAN, INF, 0.0, -10.0):
        assert call(low=v) == BAD
    assert b"lowResA" in L.thx_last_error()
    assert call(edge=NAN) == BAD and call(edge=INF) == BAD
    assert b"edgeFT" in L.thx_last_error()
    assert call(bIn=INF) == BAD and call(bIn=-INF) == BAD
    assert b"bFactorIn" in L.thx_last_error()
    for k in ("A", "B", "alpha", "fsc", "info", "fit", "sharp"):
        assert call(**{k: None}) == BAD, k
        assert b"NULL" in L.thx_last_error()
    assert call(sharp=ctypes.c_void_p(4100)) == BAD
    assert b"aligned" in L.thx_last_error()
    need = L.thx_postprocess_workspace(32, 15, 1)
    assert call(n=ctypes.c_size_t(need - 1)) == BAD
    assert b"workspace" in L.thx_last_error()
    assert call(ws=None) == BAD


def test_workspace_queries_are_host_only(L):
    for N in (15, 33, 14, 0, 1026):
        assert L.thx_postprocess_workspace(N, 5, 1) == 0
        assert L.thx_bfactor_est_workspace(N, 5) == 0
    assert L.thx_postprocess_workspace(32, 1, 1) == 0 and L.thx_postprocess_workspace(32, 17, 0) == 0
    assert L.thx_bfactor_est_workspace(32, 0) == 0 and L.thx_bfactor_est_workspace(32, 17) == 0
    # the chain works inside the FSC's workspace: no second set of volumes
    for N in (32, 256):
        ns = N // 2 - 1
        fsc = L.thx_fsc_masked_workspace(N, ns)
        assert fsc <= L.thx_postprocess_workspace(N, ns, 1) < fsc + (1 << 24)


# ------------------------------------------------------------ the restatement

def synthetic(N, c0, c1):
    """|F| = exp(c0 + c1 (u / N)^2) on shell u, random phases"""
    u = ref.shell_index(N)
    x = ((u.astype(np.float32) / np.float32(N)) ** 2).astype(np.float64)
    ph = np.exp(2j * np.pi * np.random.default_rng(4).random(u.shape))
    return np.exp(c0 + c1 * x) * ph


def test_guinier_fit_recovers_a_known_b_factor():
    for N, c0, c1 in ((32, 3.0, -40.0), (48, 1.0, -55.5), (32, 0.0, 12.0)):
        b, k0, x, y, status = ref.b_factor_est(synthetic(N, c0, c1), N // 2 - 2, 3)
        assert status == 0 and len(x) == N // 2 - 5
        assert abs(b - 2 * c1) <= 1e-12 * abs(2 * c1) and abs(k0 - c0) <= 1e-12
    assert ref.b_factor_est(synthetic(32, 0, -1), 6, 5)[4] == 1       # one shell: no fit
    F = synthetic(32, 0, -1)
    F[ref.shell_index(32) == 7] = 0
    assert ref.b_factor_est(F, 11, 3)[4] == 1                          # a shell's sum is not positive


def test_identity_filters_and_low_pass_continuity():
    F = synthetic(32, 1.0, -20.0)
    assert ref.b_factor_filter(F, 0) is F
    assert np.array_equal(ref.low_pass(F, 0.9, 0.1), F)       # thres past the corner sqrt(3) / 2
    assert ref.low_pass(F, 0.3, 0.0) is F and ref.low_pass(F, -1.0, 0.1) is F
    for dt in (np.float64, np.float32):
        th, ew = dt(0.25), dt(0.125)
        eps = 8 * np.finfo(dt).eps
        for f, v in ((th, 1.0), (th + ew, 0.0)):
            g = ref.low_pass_factor(np.array([f * (1 - eps), f, f * (1 + eps)]), th, ew, dt)
            assert np.abs(g - v).max() <= 1e-5, (dt, f, g)
        assert ref.low_pass_factor(np.array([th + ew / 2]), th, ew, dt)[0] == pytest.approx(0.5, abs=1e-6)
    out = ref.low_pass(F, 0.25, 0.125)
    f = np.sqrt(ref.freq2(32, np.float64))
    assert np.array_equal(out[f < 0.25], F[f < 0.25]) and np.all(out[f > 0.375] == 0)


def test_fsc_weight_known_answers():
    w = ref.fsc_weight(np.array([1.0, 0.0, -0.2, 0.143, 1.0 / 3.0]))
    assert w[0] == 1.0 and w[1] == 0.0 and w[2] == 0.0
    assert w[3] == pytest.approx(np.sqrt(0.286 / 1.143), rel=1e-14) and w[4] == pytest.approx(np.sqrt(0.5))
    N = 32
    F = synthetic(N, 0.0, -5.0)
    fsc = np.linspace(1.0, 0.2, 9)
    out = ref.fsc_weighting(F, fsc)
    u = ref.shell_index(N)
    assert np.all(out[u >= 9] == 0) and np.array_equal(out[u == 0], F[u == 0])
    assert np.allclose(out[u == 8], F[u == 8] * np.sqrt(0.4 / 1.2), rtol=1e-14)


@pytest.mark.parametrize("N", [32, 48, 100])
def test_shell_index_forms_agree(N):
    a, b = ref.shell_index(N), ref.shell_index_fp32(N)
    assert a.shape == (N, N, N // 2 + 1) and int((a != b).sum()) == 0


def test_merge_and_r_low():
    assert ref.r_low(32, 1.0) == 3 and ref.r_low(32, 1.6) == 5 and ref.r_low(48, 1.5) == 7
    A = np.array([1 + 2j, 3j]), np.array([3 + 0j, 1j])
    assert np.array_equal(ref.merge(*A), np.array([2 + 1j, 2j]))


@pytest.mark.parametrize("mutation", ["exponent", "inclusive", "edge", "no_sqrt"])
def test_gpu_bound_sees_one_real_mistake(mutation):
    """each mutation of the restatement moves sharp or bFactor beyond the bound
    the GPU comparison uses on this case"""
    c = pc.case(32, 1.0, 0.02)
    m = ref.postprocess(c.A, c.B, c.alpha, c.pixel_size, pc.SEED, mutate=mutation)
    e_sharp = pc.rel(m.sharp, c.ref.sharp)
    e_b = abs(m.b_factor - c.ref.b_factor) / abs(c.ref.b_factor)
    print(f"{mutation}: sharp moves {e_sharp:.3g} (bound {c.tol['sharp']:.3g}), bFactor "
          f"{e_b:.3g} (bound {c.tol['b_factor']:.3g})")
    assert e_sharp > 10 * c.tol["sharp"] or e_b > 10 * c.tol["b_factor"]


@pytest.mark.parametrize("key", list(pc.CASES))
def test_cases_reproduce_the_recorded_shells(key):
    c = pc.case(*key)
    assert (c.ref.thres, c.ref.res, c.ref.r_low) == pc.CASES[key]
    assert c.ref.status == 0 and c.ref.n_fit == c.ref.res - c.ref.r_low
    assert min(c.tol.values()) >= 1e-5


def test_degenerate_case_has_one_fit_shell():
    c = pc.case(*pc.DEGENERATE, degenerate=True)
    assert (c.ref.res, c.ref.r_low, c.ref.status, c.ref.b_factor) == (6, 5, 1, 0.0)


# ------------------------------------------------------------------- the tool

def test_fsc_file_line_format(tmp_path):
    from thunder_amd import postprocess
    p = postprocess.write_fsc(tmp_path / "Postprocess_FSC.txt", [1.0, 0.987654321, -0.25, 0.5], 32, 1.5)
    assert open(p).read() == ("00001     0.020833     0.987654\n"
                              "00002     0.041667    -0.250000\n"
                              "00003     0.062500     0.500000\n")


def test_run_refuses_mismatched_or_non_cubic_maps(tmp_path):
    from thunder_amd import postprocess
    for name, shape in (("a", (16, 16, 16)), ("b", (16, 16, 16)), ("m", (18, 18, 18)),
                        ("flat", (16, 16, 8))):
        io.write_mrc(tmp_path / f"{name}.mrc", np.zeros(shape, np.float32), 1.0)
    P = lambda n: str(tmp_path / f"{n}.mrc")
    with pytest.raises(ValueError, match="differ in size"):
        postprocess.run(P("a"), P("b"), P("m"), 1.0, str(tmp_path / "out"))
    with pytest.raises(ValueError, match="not cubic"):
        postprocess.run(P("a"), P("flat"), P("a"), 1.0, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
    assert postprocess.check_sizes([(16, 16, 16)] * 3) == 16
