"""Post-processing on the GPU (csrc/postprocess.hip, thunder_amd/postprocess.py)
against the float64 restatement of tests/postprocess_ref.py
(src/Postprocess.cpp:50-183).

Inputs, preconditions and bounds: tests/postprocess_cases.py.  Per quantity the
bound is max(1e-5, 4 e32), e32 being the restatement's float32 run against its
float64 run on the same inputs (printed): absolute for the FSC curves, relative
to max|ref| for sharp and average, relative to |bFactor| for bFactor and the
Guinier ordinates; t, res, rL and nFit are exact.
"""
import numpy as np
import pytest
import torch

import postprocess_cases as pc
import postprocess_ref as ref
from thunder_amd import io, mask as maskmod, postprocess
from thunder_amd._lib import check, lib
from thunder_amd.ops import _ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SHAPES = [(32, 1), (32, 2), (48, 1)]            # (N, method): 2 = the LDS column passes


def T_(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def gpu_run(c, method=1, A=None, B=None, **kw):
    return postprocess.postprocess(A if A is not None else T_(c.A), B if B is not None else T_(c.B),
                                   T_(c.alpha), c.pixel_size, seed=pc.SEED, b_factor=c.b_factor,
                                   method=method, **kw)


def check_case(c, got, what):
    r = c.ref
    assert (got.thres, got.res, got.r_low, got.n_fit) == (r.thres, r.res, r.r_low, r.n_fit), what
    assert got.status == r.status, what
    err = {k: float(np.abs(getattr(got, k).cpu().numpy() - getattr(r, k)).max()) for k in pc.CURVES}
    err["sharp"] = pc.rel(got.sharp.cpu().numpy(), r.sharp)
    err["average"] = pc.rel(got.average.cpu().numpy(), r.average)
    if r.b_factor != 0:
        err["b_factor"] = abs(got.b_factor - r.b_factor) / abs(r.b_factor)
        if len(r.y):
            g = got.guinier.cpu().numpy()
            assert g.shape == (2, r.n_fit)
            assert np.abs(g[0] - r.x).max() <= 1e-15
            err["guinier"] = float(np.abs(g[1] - r.y).max()) / abs(r.b_factor)
    else:
        assert got.b_factor == 0.0
    for k, e in err.items():
        print(f"{what}: {k} error {e:.3g} (bound {c.tol[k]:.3g}, e32 {c.e32[k]:.3g})")
    for k, e in err.items():
        assert e <= c.tol[k], (what, k, e, c.tol[k])
    assert got.resolution_A == pytest.approx(c.N * c.pixel_size / r.res)


@pytest.mark.parametrize("key", list(pc.CASES))
def test_chain_matches_the_reference(key):
    c = pc.case(*key)
    for N, method in SHAPES:
        if N == c.N:
            check_case(c, gpu_run(c, method), f"{c.name} method={method}")


def test_given_b_factor_skips_the_estimate():
    c = pc.case(32, 1.0, 0.05, b_factor=-60.0)
    got = gpu_run(c)
    assert got.b_factor == -60.0 and got.n_fit == 0 and got.guinier.shape == (2, 0)
    check_case(c, got, c.name)
    # the same map as from the stage entry points with that value
    est = pc.case(32, 1.0, 0.05)
    A, B = T_(c.A), T_(c.B)
    F = torch.empty_like(A)
    check(lib().thx_ft_merge_weight(_ptr(A), _ptr(B), 32, _ptr(got.fsc), 15, _ptr(F), None))
    F = postprocess.ft_sharpen(F, -60.0, got.res / 32.0, 4.0 / 32.0)
    rl = np.fft.irfftn(F.cpu().numpy().astype(np.complex128), s=(32, 32, 32), axes=(0, 1, 2))
    e = pc.rel(got.sharp.cpu().numpy(), rl * c.alpha.astype(np.float64))
    print(f"given b: chain against the stages, relative {e:.3g}")
    assert e <= c.tol["sharp"] and got.res == est.ref.res


def test_degenerate_fit_sharpens_nothing_and_says_so():
    c = pc.case(*pc.DEGENERATE, degenerate=True)
    got = gpu_run(c)
    assert got.status == 1 and got.b_factor == 0.0 and got.n_fit == 1
    check_case(c, got, c.name)


def test_inputs_untouched_and_runs_identical():
    c = pc.case(32, 1.0, 0.05)
    A, B = T_(c.A), T_(c.B)
    one = gpu_run(c, 1, A=A, B=B)
    assert torch.equal(A, T_(c.A)) and torch.equal(B, T_(c.B))
    two = gpu_run(c, 1, A=A, B=B)
    for k in pc.CURVES + ("guinier", "average", "sharp"):
        assert torch.equal(getattr(one, k), getattr(two, k)), k
    assert one[4:10] == two[4:10]
    other = gpu_run(c, 2, A=A, B=B)
    assert (other.thres, other.res, other.n_fit) == (one.thres, one.res, one.n_fit)
    e = pc.rel(other.sharp.cpu().numpy(), one.sharp.cpu().numpy().astype(np.float64))
    print(f"methods 1 and 2: sharp differs by {e:.3g} of its maximum")
    assert e <= c.tol["sharp"]
    assert abs(other.b_factor - one.b_factor) <= c.tol["b_factor"] * abs(one.b_factor)
    assert gpu_run(c, 1, A=A, B=B, want_average=False).average is None


# ----------------------------------------------------------- stage entry points

def test_merge_weight_modes():
    N, ns = 32, 15
    c = pc.case(32, 1.0, 0.05)
    A, B = T_(c.A), T_(c.B)
    fsc = T_(np.concatenate([c.ref.fsc[:12], [-0.3, 0.0, 1.0]]))
    L = lib()

    def run(a, b, f, dst):
        check(L.thx_ft_merge_weight(_ptr(a), _ptr(b), N, _ptr(f), ns, _ptr(dst), None))
        return dst.cpu().numpy()
    a64, b64 = c.A.astype(np.complex128), c.B.astype(np.complex128)
    assert np.array_equal(run(A, None, None, torch.empty_like(A)), c.A)          # a copy
    m = run(A, B, None, torch.empty_like(A))
    half = np.float32(0.5)              # exact in FP32, as the kernel's / 2
    assert np.array_equal(m.real, (c.A.real + c.B.real) * half)
    assert np.array_equal(m.imag, (c.A.imag + c.B.imag) * half)
    w = run(A, B, fsc, torch.empty_like(A))
    want = ref.fsc_weighting(ref.merge(a64, b64), fsc.cpu().numpy())
    assert pc.rel(w, want) <= 1e-6
    u = ref.shell_index(N)
    assert np.all(w[u >= ns] == 0) and np.all(w[u == 12] == 0) and np.all(w[u == 13] == 0)
    assert np.array_equal(w[u == 14], m[u == 14])                                 # weight exactly 1
    # exactly the FP32 product with the FP32 weight
    wt = ref.fsc_weight(fsc.cpu().numpy(), np.float32)
    k = u < ns
    assert np.array_equal(w[k].real, m[k].real * wt[u[k]]) and np.array_equal(w[k].imag,
                                                                                m[k].imag * wt[u[k]])
    inplace = A.clone()
    assert np.array_equal(run(inplace, B, fsc, inplace), w)
    odd = torch.empty(A.numel() + 1, dtype=A.dtype, device=DEV)[1:].view_as(A)   # 8-byte aligned only
    odd.copy_(A)
    assert np.array_equal(run(odd, B, fsc, torch.empty_like(A)), w)


def bfactor_est_case(N, rL, rU):
    """the fit over [rL, rU) of a generated spectrum against ref.b_factor_est: host rU and
    rUdev under a table of N / 2, with and without w; returns (F, u, run) to go on with"""
    rng = np.random.default_rng(8)
    u = ref.shell_index(N)
    F = (np.exp(2.0 - 30.0 * (u / N) ** 2) * (1 + 0.2 * rng.random(u.shape))
         * np.exp(2j * np.pi * rng.random(u.shape))).astype(np.complex64)
    w = 0.5 + rng.random(N // 2)
    L = lib()
    ws = torch.empty(L.thx_bfactor_est_workspace(N, N // 2), dtype=torch.uint8, device=DEV)

    def run(Fd, cap, r_dev, wd):
        out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
        g = torch.full((2, cap), -7.0, dtype=torch.float64, device=DEV)
        check(L.thx_bfactor_est(_ptr(Fd), N, rL, cap, _ptr(r_dev), _ptr(wd), _ptr(out), _ptr(g),
                                _ptr(ws), ws.numel(), None))
        return out.cpu().numpy(), g.cpu().numpy()
    Fd = T_(F)
    F64 = F.astype(np.complex128)
    for wd in (None, w):
        Fw = F64 if wd is None else F64 * np.concatenate([w, np.zeros(N // 2)])[np.minimum(u, N // 2)]
        b, c0, x, y, status = ref.b_factor_est(Fw, rU, rL)
        assert status == 0
        wt = None if wd is None else T_(w)
        for out, g in (run(Fd, rU, None, wt),
                       run(Fd, N // 2, torch.tensor([rU], dtype=torch.int32, device=DEV), wt)):
            print(f"N={N} w={'yes' if wd is not None else 'no'}: bFactor {out[0]:.6f} ref {b:.6f}")
            assert out[2] == rU - rL and out[3] == 0
            assert abs(out[0] - b) <= 1e-5 * abs(b) and abs(out[1] - c0) <= 1e-5 * abs(b)
            assert np.abs(g[0, :rU - rL] - x).max() <= 1e-15
            assert np.abs(g[1, :rU - rL] - y).max() <= 1e-5 * abs(b)
            assert np.all(g[:, rU - rL:] == 0)
    return F, u, run


def test_bfactor_est_smallest_box():
    """N = 16, rL = 1, rU = 7: host rU and rUdev, with and without w"""
    F, u, run = bfactor_est_case(16, 1, 7)
    out, _ = run(T_(F), 2, None, None)              # rU - rL = 1: no fit
    assert out[0] == 0 and out[3] == 1
    out, _ = run(T_(np.where(u == 3, 0, F).astype(np.complex64)), 7, None, None)
    assert out[0] == 0 and out[3] == 1              # a fit shell's sum is not positive


def test_bfactor_est_rows_longer_than_one_wave():
    """N = 144, rL = 1, rU = 72: a row stores 73 voxels, so the sums take the second 64-lane
    chunk of every row, whose lanes feed shells 64 .. 71"""
    bfactor_est_case(144, 1, 72)


@pytest.mark.parametrize("mode", ["b", "lowpass", "both"])
def test_sharpen_against_the_closed_form_past_one_grid_trip(mode):
    """N = 128: 128^2 65 / 2 pairs of voxels exceed the 2048 x 256 lanes of the
    capped grid, so the grid-stride loop makes a second trip"""
    N = 128
    assert N * N * (N // 2 + 1) // 2 > 2048 * 256
    rng = np.random.default_rng(2)
    F = (rng.standard_normal((N, N, N // 2 + 1)) + 1j * rng.standard_normal((N, N, N // 2 + 1))
         ).astype(np.complex64)
    b = -90.0 if mode != "lowpass" else 0.0
    shell, ew = 40, (4.0 / N if mode != "b" else 0.0)
    thres = np.float32(shell) / np.float32(N)
    f2 = ref.freq2(N, np.float32)       # the reference's f^2 and norm are RFLOATs
    f = np.sqrt(f2)
    factor = np.exp(-0.5 * b * f2.astype(np.float64))
    hi = np.float32(thres) + np.float32(ew)
    if mode != "b":
        factor = factor * ref.low_pass_factor(f.astype(np.float64), float(thres), float(hi - thres))
    want = F.astype(np.complex128) * factor
    Fd = T_(F)
    host = postprocess.ft_sharpen(Fd, b, float(thres), ew)
    e = pc.rel(host.cpu().numpy(), want)
    print(f"sharpen {mode}: relative error {e:.3g}")
    assert e <= 1e-5
    if mode != "b":
        got = host.cpu().numpy()
        assert np.all(got[f > hi] == 0) and (f > hi).any()
        if mode == "lowpass":
            assert np.array_equal(got[f < thres], F[f < thres])
    dev = postprocess.ft_sharpen(Fd, torch.tensor([b], dtype=torch.float64, device=DEV),
                                 torch.tensor([shell], dtype=torch.int32, device=DEV), ew)
    assert torch.equal(dev, host)
    inplace = Fd.clone()
    assert torch.equal(postprocess.ft_sharpen(inplace, b, float(thres), ew, out=inplace), host)


@pytest.mark.parametrize("N", [32, 48])
def test_low_pass_and_b_factor_tools(N):
    c = pc.case(N, 1.0, 0.05)
    v = c.a
    F = np.fft.rfftn(v.astype(np.float64))
    px, freq = 1.3, 6.0
    want = ref.to_real(ref.low_pass(F, np.float32(px) / np.float32(freq), 2.0 / N), N)
    got = postprocess.low_pass(T_(v), px, freq).cpu().numpy()
    e = pc.rel(got, want)
    print(f"low_pass N={N}: {e:.3g}")
    assert e <= 1e-5
    # b > 0 damps: the result is not dominated by amplified corner noise, where the forward
    # transform's FP32 error (relative to the map's norm, not to each coefficient) would be too
    want = ref.to_real(ref.b_factor_filter(F, 70.0), N)
    got = postprocess.b_factor_filter(T_(v), 70.0).cpu().numpy()
    e = pc.rel(got, want)
    print(f"b_factor_filter N={N}: {e:.3g}")
    assert e <= 1e-5
    assert pc.rel(postprocess.b_factor_filter(T_(v), 0.0).cpu().numpy(), v.astype(np.float64)) <= 1e-5


def test_run_end_to_end(tmp_path):
    N, px = 32, 1.6
    c = pc.case(N, px, 0.05)
    for name, v in (("a", c.a), ("b", c.b)):
        io.write_mrc(tmp_path / f"{name}.mrc", np.fft.fftshift(v), px)
    maskmod.save_mask(str(tmp_path / "m.mrc"), c.alpha, px)
    out = tmp_path / "out"
    r = postprocess.run(str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), str(tmp_path / "m.mrc"), px,
                        str(out), seed=pc.SEED, method=1)
    # the halves went through float32 real maps here: the shells and the B-factor still agree
    assert (r.thres, r.res, r.r_low, r.n_fit) == (c.ref.thres, c.ref.res, c.ref.r_low, c.ref.n_fit)
    assert abs(r.b_factor - c.ref.b_factor) <= 1e-4 * abs(c.ref.b_factor)
    assert pc.rel(r.sharp.cpu().numpy(), c.ref.sharp) <= 1e-4
    for name, t in (("Reference_Average.mrc", r.average), ("Reference_Sharp.mrc", r.sharp)):
        h, data = io.read_mrc(out / name)
        assert h.pixel_size == pytest.approx(px)
        assert np.array_equal(np.asarray(data), np.fft.fftshift(t.cpu().numpy()))
    rows = np.loadtxt(out / "Postprocess_FSC.txt")
    fsc = r.fsc.cpu().numpy()
    assert rows.shape == (c.n_shell - 1, 3)
    assert np.array_equal(rows[:, 0], np.arange(1, c.n_shell))
    assert np.abs(rows[:, 1] - np.arange(1, c.n_shell) / (N * px)).max() <= 1e-6
    assert np.abs(rows[:, 2] - fsc[1:]).max() <= 1e-6      # six decimals
