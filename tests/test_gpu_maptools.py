"""The map tools on the GPU (csrc/maptools.hip, thunder_amd/maptools.py) against the float64
restatement of tests/maptools_ref.py.

Inputs and bounds: tests/maptools_cases.py.  Per compared array the bound is max(1e-5, 4 e32)
relative to max|ref|, e32 being the restatement's float32 run against its float64 run on the same
input (printed with the error); permutations, copies, moves and rolls are bit-exact.  The library
is called directly with its outputs pre-filled with NaN, so an element a kernel skips shows; the
Python front end is then held to those results bit for bit.

Tie rule of the transform: under a generic matrix and an integer r, a voxel with i^2 + j^2 + k^2
= r^2 has |M x|^2 = r^2 up to rounding and may land on either side of the strict compare.  With
one matrix such a voxel must be 0 or the interpolated (or nearest) value; with many (the 59
elements of I) it must lie between the source plus the negative and the source plus the positive
ones of the 59 interpolated values, any subset of which may have been added.  The voxels so excused are counted and must stay under 2 % of
the box; at a half-integer r there are none and nothing is excused.
"""
import re

import numpy as np
import pytest
import torch

import maptools_cases as mc
import maptools_ref as ref
from thunder_amd import io, maptools, ops
from thunder_amd._lib import check, lib
from thunder_amd.ops import _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")


def T_(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def same_bytes(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


# ------------------------------------------------- the library, NaN-filled outputs
def raw_transform(vol, mats, r, interp=1, add=False):
    N = vol.shape[0]
    m = T_(np.asarray(mats, np.float64).reshape(-1, 9))
    out = torch.full_like(vol, NAN)
    check(lib().thx_vol_transform_rl(_ptr(vol), N, _ptr(m) if len(m) else None, len(m), float(r),
                                     interp, int(add), _ptr(out), _stream(DEV)), "thx_vol_transform_rl")
    return out


def raw_ft_resize(ft, M):
    out = torch.full((M, M, M // 2 + 1), complex(NAN, NAN), dtype=torch.complex64, device=DEV)
    check(lib().thx_ft_resize(_ptr(ft), ft.shape[0], _ptr(out), M, _stream(DEV)), "thx_ft_resize")
    return out


def raw_resize(vol, M):
    N = vol.shape[0]
    out = torch.full((M, M, M), NAN, dtype=torch.float32, device=DEV)
    need = lib().thx_vol_resize_workspace(N, M)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    check(lib().thx_vol_resize(_ptr(vol), N, _ptr(out), M, _ptr(ws), need, _stream(DEV)),
          "thx_vol_resize")
    return out


def raw_project(P, mat9, N, r, trans=None, want_ft=True, want_rl=True, centred=False, pf=2):
    n = len(mat9)
    m = T_(np.asarray(mat9, np.float64).reshape(n, 9))
    t = None if trans is None else T_(np.asarray(trans, np.float64))
    ft = torch.full((n, N, N // 2 + 1), complex(NAN, NAN), dtype=torch.complex64,
                    device=DEV) if want_ft else None
    rl = torch.full((n, N, N), NAN, dtype=torch.float32, device=DEV) if want_rl else None
    need = lib().thx_project_images_workspace(n, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    check(lib().thx_project_images(_ptr(P), P.shape[0], pf, _ptr(m), _ptr(t), n, N, r, _ptr(ft),
                                   _ptr(rl), int(centred), _ptr(ws), need, _stream(DEV)),
          "thx_project_images")
    return ft, rl


def raw_soft_mask(vol, r, ew, out=None):
    out = torch.full_like(vol, NAN) if out is None else out
    check(lib().thx_vol_soft_mask(_ptr(vol), vol.shape[0], float(r), float(ew), _ptr(out),
                                  _stream(DEV)), "thx_vol_soft_mask")
    return out


def rotmat_layout(mats):
    """[n, 3, 3] (x' = M x) -> [n, 9] as thx_rotmat stores a matrix (column-major)"""
    return np.asarray(mats, np.float64).reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)


# ------------------------------------------------------------------ transform
RADII = [lambda N: N // 2 - 1, lambda N: N // 2 - 1.5, lambda N: 1.5]


@pytest.mark.parametrize("N", [16, 20])
@pytest.mark.parametrize("ri", [0, 1, 2])
def test_transform_exact_cases(N, ri):
    """identity, the quarter turns about each axis (lattice points at exactly |x| = r are 0), the
    C4 elements with the source added, nearest interpolation, and no matrix at all"""
    r = RADII[ri](N)
    v = mc.volume(N)
    vol = T_(v)
    inside = ref.ball(N, r)
    for M in [np.eye(3), *mc.axis_turns()]:
        want = np.where(inside, ref.permuted(v, M), np.float32(0))
        for interp in (1, 0):
            got = raw_transform(vol, M, r, interp).cpu().numpy()
            assert np.array_equal(got, want), (N, r, interp, M)
    want = v.copy()
    for M in mc.c4_elements():
        want = want + np.where(inside, ref.permuted(v, M), np.float32(0))
    assert want.dtype == np.float32
    assert np.array_equal(raw_transform(vol, mc.c4_elements(), r, 1, add=True).cpu().numpy(), want)
    assert np.array_equal(raw_transform(vol, np.zeros((0, 3, 3)), r, 1, add=True).cpu().numpy(), v)
    assert not raw_transform(vol, np.zeros((0, 3, 3)), r, 1, add=False).cpu().numpy().any()


@pytest.mark.parametrize("N", [16, 20])
@pytest.mark.parametrize("ri", [0, 1, 2])
def test_transform_generic_rotation(N, ri):
    r = RADII[ri](N)
    M = mc.generic_mats(1, mc.RNG_MAT + N + ri)
    vol = T_(mc.volume(N))
    tie = ref.lattice_ties(N, r)
    got = raw_transform(vol, M, r).cpu().numpy()
    c_out = mc.transform_case(N, M, r, ties="out", tag=f"seed+{N + ri}")
    mc.check(c_out, "out", got, excused=tie)
    n_tie = int(tie.sum())
    print(f"N={N} r={r}: {n_tie} voxels at exactly |x| = r ({100 * n_tie / N ** 3:.2f} % of the box)")
    assert n_tie <= 0.02 * N ** 3
    if float(r).is_integer():
        assert n_tie == {(16, 7): 54, (20, 9): 102}[(N, int(r))]
        c_in = mc.transform_case(N, M, r, ties="in", tag=f"seed+{N + ri}")
        w = c_in.ref["out"]
        ok = (got == 0) | (np.abs(got - w) <= c_in.tol["out"] * np.abs(w).max())
        assert np.all(ok[tie]), "a tie voxel is neither 0 nor the interpolated value"
    else:
        assert n_tie == 0
    # nearest: the tap is chosen from the float32 coordinate, as in the restatement's float32
    # run, so the value is the same element of the source; a tie voxel holds 0 or that element
    near = raw_transform(vol, M, r, 0).cpu().numpy()
    w_out = ref.transform(mc.volume(N), M, r, "nearest", dtype=np.float32, ties="out")
    w_in = ref.transform(mc.volume(N), M, r, "nearest", dtype=np.float32, ties="in")
    assert np.array_equal(near[~tie], w_out[~tie])
    assert np.all((near[tie] == 0) | (near[tie] == w_in[tie]))


def test_transform_icosahedral_symmetrisation():
    N, r = 16, 7
    R, _ = ops.symmetry("I1")
    assert R.shape == (59, 3, 3)
    vol = T_(mc.volume(N))
    got = raw_transform(vol, R, r, 1, add=True)
    tie = ref.lattice_ties(N, r)
    assert int(tie.sum()) == 54 and tie.sum() <= 0.02 * N ** 3
    c = mc.transform_case(N, R, r, add_src=True, ties="out", tag="I1")
    g = got.cpu().numpy()
    mc.check(c, "out", g, excused=tie)
    # a tie voxel holds the source plus any subset of the 59 interpolated values: between the
    # source plus the negative ones and the source plus the positive ones
    v = mc.volume(N).astype(np.float64)
    each = np.stack([ref.transform(v, M, r, ties="in")[tie] for M in R])
    lo, hi = v[tie] + np.minimum(each, 0).sum(0), v[tie] + np.maximum(each, 0).sum(0)
    slack = c.tol["out"] * np.abs(c.ref["out"]).max()
    print(f"I1 tie voxels: span of the bracket {float((hi - lo).max()):.3g}, slack {slack:.3g}")
    assert np.all((g[tie] >= lo - slack) & (g[tie] <= hi + slack))
    assert same_bytes(maptools.symmetrize(vol, "I1"), got)


# --------------------------------------------------------------------- resize
PAIRS = [(16, 32), (32, 16), (16, 24), (24, 16), (16, 16)]


@pytest.mark.parametrize("N, M", PAIRS)
def test_ft_resize_is_a_move(N, M):
    ft = np.fft.rfftn(mc.volume(N).astype(np.float64)).astype(np.complex64)
    got = raw_ft_resize(T_(ft), M)
    assert np.array_equal(got.cpu().numpy(), ref.ft_resize(ft, M))
    assert same_bytes(maptools.ft_resize(T_(ft), M), got)


@pytest.mark.parametrize("N, M", PAIRS)
def test_vol_resize(N, M):
    vol = T_(mc.volume(N))
    got = raw_resize(vol, M)
    c = mc.resize_case(N, M)
    mc.check(c, "out", got.cpu().numpy())
    if N == M:
        print("16 -> 16 against the input:", mc.rel(got.cpu().numpy(), mc.volume(N).astype(np.float64)))
        assert mc.rel(got.cpu().numpy(), mc.volume(N).astype(np.float64)) <= c.tol["out"]
    assert torch.equal(vol, T_(mc.volume(N))), "src was written"
    assert same_bytes(maptools.resize(vol, M), got)


# -------------------------------------------------------------------- project
@pytest.mark.parametrize("r", [7, 3])
def test_projection_at_the_identity_is_exact(r):
    N, pf = 16, 2
    P = mc.projectee(N, pf)
    ft, rl = raw_project(T_(P), np.eye(3).reshape(1, 9), N, r)
    j, i = np.meshgrid(ref.signed(N), np.arange(N // 2 + 1), indexing="ij")
    want = np.where(i * i + j * j < r * r, P[0][(pf * j) % (pf * N), pf * i], np.complex64(0))
    assert np.array_equal(ft[0].cpu().numpy(), want)
    assert np.all(np.isfinite(rl.cpu().numpy()))


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("r", [7, 3])
@pytest.mark.parametrize("with_trans", [False, True])
def test_projection_generic(n, r, with_trans):
    N = 16
    c = mc.project_case(N, n, r, with_trans)
    P = T_(mc.projectee(N))
    m9 = rotmat_layout(c.mats)
    ft, rl = raw_project(P, m9, N, r, c.trans)
    mc.check(c, "ft", ft.cpu().numpy())
    mc.check(c, "rl", rl.cpu().numpy())
    j, i = np.meshgrid(ref.signed(N), np.arange(N // 2 + 1), indexing="ij")
    outside = ~(i * i + j * j < r * r)
    assert not ft.cpu().numpy()[:, outside].any(), "a pixel outside the disc is not 0"
    # one output at a time, and the centred layout: the same bytes, rolled
    only_ft, none = raw_project(P, m9, N, r, c.trans, want_rl=False)
    assert none is None and same_bytes(only_ft, ft)
    none, only_rl = raw_project(P, m9, N, r, c.trans, want_ft=False)
    assert none is None and same_bytes(only_rl, rl)
    _, cen = raw_project(P, m9, N, r, c.trans, want_ft=False, centred=True)
    assert same_bytes(cen, torch.roll(rl, (N // 2, N // 2), (1, 2)))
    # the front end: matrices, both outputs
    t = None if c.trans is None else T_(c.trans)
    a_rl, a_ft = maptools.project(P, T_(m9), N, r=r, trans=t, ft=True)
    assert same_bytes(a_rl, rl) and same_bytes(a_ft, ft)


def test_projection_from_quaternions_and_empty_batch():
    N = 16
    P = T_(mc.projectee(N))
    c = mc.project_case(N, 3, 7, False)             # its matrices are those of these quaternions
    q = T_(mc.generic_quats(3, mc.RNG_MAT + 3))
    rl = maptools.project(P, q, N)
    assert same_bytes(rl, maptools.project(P, ops.rotmat(q), N))
    mc.check(c, "rl", rl.cpu().numpy())
    empty = maptools.project(P, q[:0], N, ft=True)
    assert empty[0].shape == (0, N, N) and empty[1].shape == (0, N, N // 2 + 1)


# ------------------------------------------------------------------ soft mask
@pytest.mark.parametrize("ew", [2.0, 6.0])
def test_soft_mask(ew):
    N, r = 16, 5.0
    vol = T_(mc.volume(N))
    got = raw_soft_mask(vol, r, ew)
    mc.check(mc.soft_mask_case(N, r, ew), "out", got.cpu().numpy())
    k, j, i = ref.grid3(N)
    u2 = i * i + j * j + k * k
    g = got.cpu().numpy()
    assert np.array_equal(g[u2 < r * r], mc.volume(N)[u2 < r * r])
    assert not g[u2 > (r + ew) ** 2].any()
    work = vol.clone()
    assert raw_soft_mask(work, r, ew, out=work) is work and same_bytes(work, got)
    assert same_bytes(maptools.soft_mask(vol, r, ew), got)


# -------------------------------------------------------- tools, determinism
def write_centred(path, v, pixel_size=1.5):
    io.write_mrc(str(path), np.fft.fftshift(v), pixel_size)
    return str(path)


def read_centred(path):
    return np.fft.ifftshift(np.asarray(io.read_mrc(str(path))[1], np.float32))


def test_map_tools_through_files(tmp_path):
    N = 16
    v, w = mc.volume(N), mc.volume(N)[::-1].copy()
    a, b = write_centred(tmp_path / "a.mrc", v), write_centred(tmp_path / "b.mrc", w)
    va, vb = T_(v), T_(w)
    out = str(tmp_path / "out.mrc")
    for run, want in [
            (lambda: maptools.run_resize(a, out, 24, 1.5), maptools.resize(va, 24)),
            (lambda: maptools.run_align_z(a, out, (1, 2, 2), 1.5), maptools.align_z(va, (1, 2, 2))),
            (lambda: maptools.run_mask(a, out, 5, 1.5), maptools.soft_mask(va, 5, 6)),
            (lambda: maptools.run_average(a, b, out, 1.5), maptools.average(va, vb)),
            (lambda: maptools.run_minus(a, b, out, 1.5), maptools.minus(va, vb))]:
        ret = run()
        assert same_bytes(ret, want)
        assert np.array_equal(read_centred(out), want.cpu().numpy())
        assert io.read_mrc(out)[0].pixel_size == pytest.approx(1.5)
    assert np.array_equal(maptools.average(va, vb).cpu().numpy(), (v + w) / np.float32(2))
    assert np.array_equal(maptools.minus(va, vb).cpu().numpy(), v - w)
    # align_z normalises: a vector and its multiples give the same map
    assert same_bytes(maptools.align_z(va, (1, 2, 2)), maptools.align_z(va, (0.5, 1, 1)))
    M = maptools.align_z_matrix(np.array([1, 2, 2]) / 3.0)
    assert same_bytes(maptools.align_z(va, (1, 2, 2)), raw_transform(va, M, N // 2 - 1))


def test_run_project_stack_and_metadata(tmp_path):
    N, seed = 16, 5
    inp = write_centred(tmp_path / "ref.mrc", mc.volume(N))
    out, meta = str(tmp_path / "proj"), str(tmp_path / "meta.txt")
    quats = []
    for rank in (0, 1):
        stack, q = maptools.run_project(inp, out, meta, 5, 1.5, seed, rank=rank, world=2, chunk=1)
        assert stack == "%s_Rank_%06d.mrcs" % (out, rank) and q.shape == (2, 4)   # 5 -> 4 -> 2 each
        quats.append(q)
    q = np.concatenate(quats)
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-12 and len(np.unique(q, axis=0)) == 4
    lines = open(meta).read().splitlines()
    assert len(lines) == 4
    num = r" +(-?\d+\.\d{9})"
    for n, line in enumerate(lines):
        rank, l = divmod(n, 2)
        m = re.fullmatch(r"(\d{12})@(\S+)" + num * 4, line)
        assert m and int(m.group(1)) == l and m.group(2) == "%s_Rank_%06d.mrcs" % (out, rank)
        assert line == "%012d@%s_Rank_%06d.mrcs %18.9f %18.9f %18.9f %18.9f" % (l, out, rank, *q[n])
    # the stacks hold the API's projections of those quaternions, centred
    from thunder_amd import reference
    P = reference.refresh_projectee(T_(mc.volume(N)), pf=2)
    want = maptools.project(P, T_(q), N, centred=True).cpu().numpy()
    for rank in (0, 1):
        h, data = io.read_mrc("%s_Rank_%06d.mrcs" % (out, rank))
        assert data.shape == (2, N, N) and np.array_equal(np.asarray(data), want[2 * rank:2 * rank + 2])
    # chunking does not change a byte, and the same seed gives the same run
    again, q2 = maptools.run_project(inp, str(tmp_path / "again"), str(tmp_path / "m2.txt"), 4, 1.5,
                                     seed, chunk=3)
    assert np.array_equal(q2, q)
    assert np.array_equal(np.asarray(io.read_mrc(again)[1]), want)


def test_every_entry_point_is_deterministic():
    N = 16
    vol, P = T_(mc.volume(N)), T_(mc.projectee(N))
    R, _ = ops.symmetry("I1")
    ft = T_(np.fft.rfftn(mc.volume(N).astype(np.float64)).astype(np.complex64))
    m9 = rotmat_layout(mc.generic_mats(65))
    trans = np.random.default_rng(3).uniform(-3, 3, (65, 2))
    calls = [lambda: raw_transform(vol, R, 7, 1, add=True),
             lambda: raw_transform(vol, mc.generic_mats(1), 6.5, 0),
             lambda: raw_ft_resize(ft, 24), lambda: raw_resize(vol, 24), lambda: raw_resize(vol, 16),
             lambda: raw_project(P, m9, N, 7, trans)[0], lambda: raw_project(P, m9, N, 7, trans)[1],
             lambda: raw_soft_mask(vol, 5, 6)]
    for n, call in enumerate(calls):
        assert same_bytes(call(), call()), n
