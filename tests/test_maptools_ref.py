"""The float64 restatement of the map tools (tests/maptools_ref.py) against closed forms, to
1e-12 unless exact.  No device is needed."""
import numpy as np
import pytest

import maptools_cases as cases
import maptools_ref as ref


def affine(N, a=0.3, b=(0.7, -1.1, 0.45)):
    k, j, i = ref.grid3(N)
    return a + b[0] * i + b[1] * j + b[2] * k


@pytest.mark.parametrize("N, r", [(16, 6.0), (16, 5.5), (20, 8.5)])
def test_trilinear_reproduces_an_affine_field(N, r):
    """a + b.x under a generic rotation is a + b.(M x) inside the ball and 0 outside; the taps
    stay away from the box faces (r <= N/2 - 2), where the wrapped field jumps"""
    a, b = 0.3, np.array([0.7, -1.1, 0.45])
    M = cases.generic_mats(1)[0]
    out = ref.transform(affine(N, a, b), M, r)
    k, j, i = ref.grid3(N)
    x, y, z, q2 = ref.rotated(M, i, j, k)
    want = np.where(q2 < r * r, a + b[0] * x + b[1] * y + b[2] * z, 0.0)
    assert np.abs(out - want).max() < 1e-12


permuted = ref.permuted


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identity_and_signed_permutations_are_exact(dtype):
    N, r = 16, 7
    v = cases.volume(N)
    inside = ref.ball(N, r)
    assert inside.sum() < N ** 3 and ref.lattice_ties(N, r).sum() == 54
    for M in [np.eye(3), *cases.axis_turns(), -np.eye(3)]:
        for interp in ("linear", "nearest"):
            out = ref.transform(v, M, r, interp, dtype=dtype)
            assert np.array_equal(out, np.where(inside, permuted(v, M), 0).astype(dtype))
    # the C4 elements with the source added: the permuted copies summed in index order
    want = v.astype(dtype)
    for M in cases.c4_elements():
        want = (want + np.where(inside, permuted(v, M), 0).astype(dtype)).astype(dtype)
    assert np.array_equal(ref.transform(v, cases.c4_elements(), r, add_src=True, dtype=dtype), want)
    # no matrix: a copy or a clear
    assert np.array_equal(ref.transform(v, np.zeros((0, 3, 3)), r, add_src=True), v)
    assert not ref.transform(v, np.zeros((0, 3, 3)), r).any()


def test_tie_counts():
    """the lattice points at exactly |x| = r: the issue's counts, and none for a half-integer r"""
    assert ref.lattice_ties(16, 7).sum() == 54 and ref.lattice_ties(20, 9).sum() == 102
    assert ref.lattice_ties(16, 6.5).sum() == 0 and ref.lattice_ties(16, 1.5).sum() == 0


def test_ft_resize_round_trip_is_exact():
    ft = np.fft.rfftn(cases.volume(16).astype(np.float64)).astype(np.complex64)
    up = ref.ft_resize(ft, 32)
    assert up.shape == (32, 32, 17) and np.array_equal(ref.ft_resize(up, 16), ft)
    assert np.array_equal(ref.ft_resize(ft, 16), ft)
    # only the common cube is populated, the row j = -L/2 at its own place
    assert np.count_nonzero(up) == np.count_nonzero(ft)
    assert np.array_equal(up[0, 32 - 8, :9], ft[0, 8, :]) and not up[0, 8, :].any()


@pytest.mark.parametrize("N, M", [(16, 32), (32, 16), (16, 24), (24, 16)])
def test_plane_wave_resizes_to_its_scaled_self(N, M):
    u = np.array([2, -3, 1])            # (u_i, u_j, u_k), every |u_c| < min(N, M) / 2
    k, j, i = ref.grid3(N)
    v = np.cos(2 * np.pi * (u[0] * i + u[1] * j + u[2] * k) / N)
    k, j, i = ref.grid3(M)
    want = (N / M) ** 3 * np.cos(2 * np.pi * (u[0] * i + u[1] * j + u[2] * k) / M)
    assert np.abs(ref.resize(v, M) - want).max() < 1e-12
    # the mean is (N / M)^3 times the input's: nothing is renormalised
    w = cases.volume(N).astype(np.float64)
    assert abs(ref.resize(w, M).mean() - (N / M) ** 3 * w.mean()) < 1e-12


def test_projection_at_the_identity_is_the_central_plane():
    N, pf = 16, 2
    P = cases.projectee(N, pf)
    for r in (7, 3):
        ft, rl = ref.project(P, np.eye(3)[None], N, pf, r)
        j, i = np.meshgrid(ref.signed(N), np.arange(N // 2 + 1), indexing="ij")
        disc = i * i + j * j < r * r
        want = np.where(disc, P[0][(pf * j) % (pf * N), pf * i], 0)
        assert np.array_equal(ft[0], want.astype(np.complex128))
        assert rl.shape == (1, N, N) and np.all(np.isfinite(rl))


def test_quarter_turn_about_z_permutes_the_projection():
    """P(R x) with R the 90 degree turn about z: pixel (i, j) reads the central plane at
    (-j, i), folded onto the stored half where -j < 0"""
    N, pf, r = 16, 2, 7
    P = cases.projectee(N, pf)
    vdim = pf * N
    ft, _ = ref.project(P, cases.axis_turns()[2][None], N, pf, r)
    j, i = np.meshgrid(ref.signed(N), np.arange(N // 2 + 1), indexing="ij")
    disc = i * i + j * j < r * r
    x, y = -pf * j, pf * i
    fold = x < 0
    val = P[0][np.where(fold, -y, y) % vdim, np.abs(x)]
    want = np.where(disc, np.where(fold, np.conj(val), val), 0)
    assert np.array_equal(ft[0], want.astype(np.complex128))


def test_translation_is_a_phase_ramp():
    N, pf = 16, 2
    P = cases.projectee(N, pf)
    M = cases.generic_mats(1)
    t = np.array([[1.25, -2.5]])
    plain, _ = ref.project(P, M, N, pf, 7)
    moved, _ = ref.project(P, M, N, pf, 7, t)
    j, i = np.meshgrid(ref.signed(N), np.arange(N // 2 + 1), indexing="ij")
    assert np.abs(moved[0] - plain[0] * np.exp(-2j * np.pi * (i * t[0, 0] + j * t[0, 1]) / N)).max() \
        < 1e-12 * np.abs(plain).max()


def test_soft_mask_profile():
    N, r, ew = 16, 5.0, 2.0
    v = np.ones((N, N, N))
    m = ref.soft_mask(v, r, ew)
    k, j, i = ref.grid3(N)
    u = np.sqrt(i * i + j * j + k * k)
    assert np.array_equal(m[u < r], v[u < r]) and not m[u > r + ew].any()
    edge = (u >= r) & (u <= r + ew)
    assert np.abs(m[edge] - (0.5 + 0.5 * np.cos((u[edge] - r) / ew * np.pi))).max() < 1e-12


@pytest.mark.parametrize("v", [(0.3, -0.5, 0.8), (0, 0, 1), (0, 1, 0), (1, 1, 1), (0.999, 0.03, 0.02)])
def test_align_z_of_a_unit_vector_is_a_rotation(v):
    from thunder_amd import maptools
    v = np.asarray(v, np.float64)
    v = v / np.linalg.norm(v)
    M = ref.align_z(v)
    assert np.abs(M @ M.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
    assert np.abs(M @ v - [0, 0, 1]).max() < 1e-12
    assert np.array_equal(maptools.align_z_matrix(v), M)


def test_align_z_degenerate_branch_and_length():
    from thunder_amd import maptools
    fixed = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])
    for v in ((1, 0, 0), (1, 0.005, 0.005), (-2, 0, 0.01)):    # within 1e-2 of the x axis
        assert np.array_equal(ref.align_z(v), fixed) and np.array_equal(maptools.align_z_matrix(v), fixed)
    assert abs(np.linalg.det(fixed) - 1) < 1e-12 and np.array_equal(fixed @ [1, 0, 0], [0, 0, 1])
    # any other length: the first row scales with |v| and the matrix is no rotation
    M = ref.align_z((0.6, -1.0, 1.6))
    assert abs(np.linalg.norm(M[0]) - np.linalg.norm((0.6, -1.0, 1.6))) < 1e-12
    assert abs(np.linalg.det(M) - 1) > 0.5
