"""The round's last stage without a GPU: the numpy restatement
(tests/refresh_ref.py) against closed forms that involve no FFT of its own --
a single voxel's projectee, the three branches of the soft mask, the low-pass
edge, the averaging on the r^2 boundary -- then the host-only workspace query
and the argument validation of csrc/refresh.hip's entry points, which has to
answer THX_ERR_ARG before anything is enqueued."""
import ctypes
import math

import numpy as np
import pytest

import refresh_ref as rr
from thunder_amd import _lib, build

vp = ctypes.c_void_p
ERR_ARG = 1


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def P(a):
    return a.ctypes.data_as(vp)


def corner_positions(N):
    """Signed voxels with each axis at -N/2 and at N/2-1 (the wrap and the
    off-by-one cases), the origin and an interior point."""
    lo, hi = -N // 2, N // 2 - 1
    return [(0, 0, 0), (lo, 0, 0), (0, lo, 0), (0, 0, lo), (hi, 0, 0), (0, hi, 0), (0, 0, hi),
            (lo, hi, 1), (hi, lo, lo), (2, -3, 1)]


@pytest.mark.parametrize("N,pf", [(8, 2), (16, 2), (8, 1)])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_single_voxel_closed_form(N, pf, interp):
    for n, pos in enumerate(corner_positions(N)):
        w = 1.0 + 0.25 * n
        src = np.zeros((N, N, N))
        src[pos[2] % N, pos[1] % N, pos[0] % N] = w
        for mr in (None, N / 4):
            got = rr.projectee(src, pf, mask_radius=mr, edge=6, interp=interp)
            ref = rr.single_voxel(N, pf, pos, w, mr, 6, interp)
            assert got.shape == (pf * N, pf * N, pf * N // 2 + 1)
            assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), (pos, mr)


def test_single_voxel_closed_form_2d():
    N, pf = 16, 2
    for pos in [(0, 0), (-N // 2, 0), (0, -N // 2), (N // 2 - 1, 0), (0, N // 2 - 1), (-8, 7), (3, -2)]:
        src = np.zeros((N, N))
        src[pos[1] % N, pos[0] % N] = 1.5
        got = rr.projectee(src, pf, mask_radius=N / 4, edge=6, dims=2)
        ref = rr.single_voxel(N, pf, pos, 1.5, N / 4, 6)
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), pos


def test_grid_correction_uses_the_padded_box():
    # |r| / (pf vdim) with vdim = pf N, not the reconstruction's |r| / (pf N)
    N, pf = 8, 2
    src = np.zeros((N, N, N))
    src[0, 0, 3] = 1.0
    got = rr.projectee(src, pf)[0, 0, 0].real
    x = math.pi * 3 / (pf * pf * N)
    assert got == pytest.approx(1.0 / (math.sin(x) / x) ** 2, rel=1e-13)
    y = math.pi * 3 / (pf * N)
    assert abs(got - 1.0 / (math.sin(y) / y) ** 2) > 1e-2


def test_soft_mask_branches():
    N, r, ew = 16, 4.0, 6.0
    src = np.full((N, N, N), 2.0)
    got = rr.soft_mask(src, r, ew)
    s = rr.signed(N)
    seen = set()
    for (k, j, i) in [(0, 0, 0), (0, 0, 3), (0, 0, 4), (0, 3, 4), (0, 0, 7), (8, 8, 8), (0, 6, 8),
                      (15, 15, 15), (0, 10, 0)]:
        u = math.sqrt(float(s[i] ** 2 + s[j] ** 2 + s[k] ** 2))
        if u > r + ew:
            want, br = 0.0, "out"
        elif u >= r:
            want, br = 2.0 * (1 - (0.5 - 0.5 * math.cos((u - r) / ew * math.pi))), "edge"
        else:
            want, br = 2.0, "in"
        seen.add(br)
        assert got[k, j, i] == pytest.approx(want, abs=1e-14), (k, j, i)
    assert seen == {"in", "edge", "out"}
    # u == r keeps the source, u == r + ew is exactly background
    assert got[0, 0, 4] == 2.0
    assert rr.soft_mask_weight(np.array([r + ew]), r, ew)[0] == pytest.approx(0.0, abs=1e-16)
    # the provided-mask form: src (1 - (1 - alpha))
    al = np.linspace(0, 1, N ** 3).reshape(N, N, N)
    assert np.allclose(rr.alpha_mask(src, al), 2.0 * al, atol=1e-15)


def test_low_pass_edge():
    N, thres, ew = 16, 0.25, 4.0 / 16
    F = np.ones((N, N, N // 2 + 1), np.complex128) * (1 + 2j)
    got = rr.low_pass(F, thres, ew)
    assert got[0, 0, 3] == 1 + 2j                         # f = 3/16 < thres
    f = 6 / 16
    assert got[0, 0, 6] == pytest.approx((1 + 2j) * (math.cos((f - thres) * math.pi / ew) / 2 + 0.5))
    assert got[0, 0, 4] == pytest.approx(1 + 2j)          # f == thres: the edge's start, weight 1
    assert got[8, 8, 8] == 0                              # f = sqrt(3)/2 > thres + ew
    f = math.sqrt(2) * 5 / 16                             # negative j, k count by their signed value
    assert got[N - 5, N - 5, 0] == pytest.approx((1 + 2j) * (math.cos((f - thres) * math.pi / ew) / 2 + 0.5))


def test_average_on_the_boundary():
    N, r = 16, 5
    rng = np.random.default_rng(3)
    shape = (N, N, N // 2 + 1)
    A = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    B = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    a, b = rr.average(A, B, r)
    # 3^2 + 4^2 + 0 == r^2: not below, unchanged; 3, 3, 2 (22 < 25) averaged
    assert a[0, 4, 3] == A[0, 4, 3] and b[0, 4, 3] == B[0, 4, 3]
    assert a[0, N - 4, 3] == A[0, N - 4, 3]
    assert a[N - 5, 0, 0] == A[N - 5, 0, 0] and a[N - 4, 0, 0] == (A[N - 4, 0, 0] + B[N - 4, 0, 0]) / 2
    assert a[2, 3, 3] == b[2, 3, 3] == (A[2, 3, 3] + B[2, 3, 3]) / 2
    n_avg = int(np.sum(a == b))
    assert n_avg == int(np.sum(rr._quad_ft(N, 3) < r * r)) and 0 < n_avg < a.size
    a, b = rr.average(A, B, None)
    assert np.array_equal(a, (A + B) / 2) and np.array_equal(a, b)
    a, b = rr.average(A, B, 0)
    assert np.array_equal(a, A) and np.array_equal(b, B)
    # 2D: QUAD(i, j)
    a2, b2 = rr.average(A[0], B[0], r, dims=2)
    assert a2[4, 3] == A[0, 4, 3] and a2[3, 3] == (A[0, 3, 3] + B[0, 3, 3]) / 2


def test_float32_restatement_is_close():
    N, pf = 16, 2
    src = np.random.default_rng(5).standard_normal((N, N, N))
    r64 = rr.projectee(src, pf, mask_radius=N / 4)
    r32 = rr.projectee(src, pf, mask_radius=N / 4, dtype=np.float32)
    assert r32.dtype == np.complex64
    e32 = np.max(np.abs(r32 - r64)) / np.max(np.abs(r64))
    assert 0 < e32 < 1e-5


# ------------------------------------------------------------ the library
def test_workspace_query_is_host_only_and_grows(L):
    for method in (0, 1, 2):
        for ft in (0, 1):
            sizes = [L.thx_projectee_workspace(N, 2, method, ft) for N in (8, 16, 32, 64, 128, 256)]
            assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])), (method, ft, sizes)
        assert L.thx_projectee_workspace(64, 2, method, 1) > L.thx_projectee_workspace(64, 2, method, 0)
    # the fallback holds the padded real volume, the pruned path never does
    assert L.thx_projectee_workspace(256, 2, 1, 0) >= 512 ** 3 * 4
    assert L.thx_projectee_workspace(256, 2, 2, 0) < 512 ** 3 * 4
    assert L.thx_projectee_workspace(256, 2, 2, 0) >= (256 * 256 + 256 * 512) * 257 * 8
    # boxes the pruned path does not serve: C4's 200, C5's 512 at pf 2
    assert L.thx_projectee_workspace(200, 2, 2, 0) == 0 and L.thx_projectee_workspace(200, 2, 0, 0) > 0
    assert L.thx_projectee_workspace(512, 2, 2, 0) == 0 and L.thx_projectee_workspace(512, 2, 0, 0) > 0
    for bad in ((0, 2, 0, 0), (6, 2, 0, 0), (33, 2, 0, 0), (32, 0, 0, 0), (32, 2, 3, 0), (32, 2, -1, 0)):
        assert L.thx_projectee_workspace(*bad) == 0, bad
    s2 = [L.thx_projectee2d_workspace(N, 2, 3, 0) for N in (16, 32, 64)]
    assert all(b > a > 0 for a, b in zip(s2, s2[1:]))
    assert L.thx_projectee2d_workspace(16, 2, 0, 0) == 0 and L.thx_projectee2d_workspace(15, 2, 3, 0) == 0


def test_projectee_rejects_bad_arguments_without_gpu(L):
    N, pf = 16, 2
    vdim = N * pf
    src = np.zeros((N, N, N), np.float32)
    al = np.ones((N, N, N), np.float32)
    dst = np.zeros((vdim, vdim, vdim // 2 + 1), np.complex64)
    need = L.thx_projectee_workspace(N, pf, 0, 1)
    ws = np.zeros(need, np.uint8)

    def call(src_=src, fromFT=0, N_=N, pf_=pf, rMask=4.0, edge=6.0, alpha=None, interp=0, scale=1.0,
             dst_=dst, method=0, ws_=ws, wsBytes=None):
        return L.thx_projectee(None if src_ is None else P(src_), fromFT, N_, pf_, rMask, edge,
                               None if alpha is None else P(alpha), interp, scale,
                               None if dst_ is None else P(dst_), method,
                               None if ws_ is None else P(ws_),
                               (0 if ws_ is None else ws_.nbytes) if wsBytes is None else wsBytes, None)

    assert call(src_=None) == ERR_ARG and call(dst_=None) == ERR_ARG
    for n in (0, 6, 15, -16):
        assert call(N_=n) == ERR_ARG, n
    assert call(pf_=0) == ERR_ARG and call(pf_=-2) == ERR_ARG
    for e in (0.0, -1.0, float("nan"), float("inf")):
        assert call(edge=e) == ERR_ARG, e
    assert call(rMask=float("nan")) == ERR_ARG and call(scale=float("inf")) == ERR_ARG
    assert call(alpha=al) == ERR_ARG                      # rMask and alphaMask together
    assert b"exclusive" in L.thx_last_error()
    assert call(interp=2) == ERR_ARG
    assert call(method=3) == ERR_ARG and call(method=-1) == ERR_ARG
    assert call(N_=24, method=2) == ERR_ARG               # pruned path: power-of-two boxes only
    assert b"pruned" in L.thx_last_error()
    assert call(ws_=None) == ERR_ARG
    assert call(wsBytes=L.thx_projectee_workspace(N, pf, 0, 0) - 1) == ERR_ARG
    assert b"workspace" in L.thx_last_error()
    assert call(fromFT=1, wsBytes=L.thx_projectee_workspace(N, pf, 0, 0)) == ERR_ARG
    # dst aliasing src, the workspace or the mask
    big = np.zeros(dst.nbytes + need, np.uint8)
    assert L.thx_projectee(P(big), 0, N, pf, 4.0, 6.0, None, 0, 1.0, P(big), 0, P(ws), ws.nbytes,
                           None) == ERR_ARG
    assert b"aliases src" in L.thx_last_error()
    assert L.thx_projectee(P(src), 0, N, pf, 4.0, 6.0, None, 0, 1.0, P(big), 0, P(big), big.nbytes,
                           None) == ERR_ARG
    assert b"aliases the workspace" in L.thx_last_error()
    assert L.thx_projectee(P(src), 0, N, pf, 0.0, 6.0, P(big), 0, 1.0, P(big), 0, P(ws), ws.nbytes,
                           None) == ERR_ARG


def test_projectee2d_and_average_reject_bad_arguments_without_gpu(L):
    N, pf, nK = 16, 2, 3
    src = np.zeros((nK, N, N), np.float32)
    dst = np.zeros((nK, N * pf, N * pf // 2 + 1), np.complex64)
    ws = np.zeros(L.thx_projectee2d_workspace(N, pf, nK, 1), np.uint8)
    ok = dict(fromFT=0, nK=nK, N=N, pf=pf, rMask=4.0, edge=6.0, alpha=None, interp=0, scale=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.thx_projectee2d(P(src), a["fromFT"], a["nK"], a["N"], a["pf"], a["rMask"], a["edge"],
                                 a["alpha"], a["interp"], a["scale"], P(dst), P(ws),
                                 a.get("wsBytes", ws.nbytes), None)

    assert call(alpha=P(src)) == ERR_ARG                  # the reference aborts on a 2D provided mask
    assert b"3D only" in L.thx_last_error()
    assert call(nK=0) == ERR_ARG and call(N=7) == ERR_ARG and call(N=4) == ERR_ARG
    assert call(pf=0) == ERR_ARG and call(edge=0.0) == ERR_ARG and call(edge=float("nan")) == ERR_ARG
    assert call(interp=-1) == ERR_ARG and call(wsBytes=16) == ERR_ARG
    assert L.thx_projectee2d(P(dst), 0, nK, N, pf, 4.0, 6.0, None, 0, 1.0, P(dst), P(ws), ws.nbytes,
                             None) == ERR_ARG

    A = np.zeros((N, N, N // 2 + 1), np.complex64)
    B = np.zeros_like(A)
    assert L.thx_ref_average(None, P(B), N, 1, 3.0, 0.0, 1.0, 1, None) == ERR_ARG
    assert L.thx_ref_average(P(A), P(A), N, 1, 3.0, 0.0, 1.0, 1, None) == ERR_ARG
    for n in (0, 6, 17):
        assert L.thx_ref_average(P(A), P(B), n, 1, 3.0, 0.0, 1.0, 1, None) == ERR_ARG
    assert L.thx_ref_average(P(A), P(B), N, 0, 3.0, 0.0, 1.0, 1, None) == ERR_ARG
    assert L.thx_ref_average(P(A), P(B), N, 1, float("nan"), 0.0, 1.0, 1, None) == ERR_ARG
    for ew in (0.0, -0.1, float("nan")):
        assert L.thx_ref_average(P(A), P(B), N, 1, 3.0, 0.25, ew, 1, None) == ERR_ARG
