"""Pins tests/mask_ref.py, the scatter-form restatement of src/Functions/
Mask.cpp:581-731 that the GPU mask tests compare against, on cases with a
closed form.  No GPU and no library needed."""
import numpy as np
import pytest

import mask_ref

N = 16


def signed_grid(n):
    ax = np.fft.fftfreq(n, 1.0 / n).astype(np.int64)
    return np.meshgrid(ax, ax, ax, indexing="ij")       # k, j, i at the stored index


def single_voxel(n, at=(0, 0, 0)):
    m = np.zeros((n, n, n), np.float32)
    m[at[0] % n, at[1] % n, at[2] % n] = 1              # at = (k, j, i), signed
    return m


@pytest.mark.parametrize("ext", [2.0, 2.5, 3.0])
def test_single_voxel_extends_to_the_open_ball(ext):
    k, j, i = signed_grid(N)
    got = mask_ref.extend(single_voxel(N), ext)
    want = (i * i + j * j + k * k < ext * ext).astype(np.float32)
    assert np.array_equal(got, want)
    # the offset -a of the grid [-a, a) is never taken: the ball is symmetric
    neg = (-np.arange(N)) % N
    assert np.array_equal(got, got[np.ix_(neg, neg, neg)])
    assert got.sum() == {2.0: 27, 2.5: 81, 3.0: 93}[ext]


@pytest.mark.parametrize("ew", [1.0, 3.5, 6.0])
def test_soft_edge_of_a_single_voxel_is_the_closed_form(ew):
    k, j, i = signed_grid(N)
    d = np.sqrt((i * i + j * j + k * k).astype(np.float64))
    got = mask_ref.soft_edge(single_voxel(N), ew)
    want = np.where((d > 0) & (d < ew), 0.5 + 0.5 * np.cos(d / ew * np.pi), single_voxel(N))
    assert np.abs(got - want).max() < 1e-6
    assert np.array_equal(got != single_voxel(N), (d > 0) & (d < ew))
    assert np.array_equal(mask_ref.soft_edge(single_voxel(N), 0.0), single_voxel(N))


@pytest.mark.parametrize("r", [2.0, 2.5])
def test_erosion_of_an_extended_ball_contains_the_original(r):
    k, j, i = signed_grid(24)
    ball = (i * i + j * j + k * k < 16).astype(np.float32)
    grown = mask_ref.extend(ball, r)
    back = mask_ref.extend(grown, -r)
    assert grown.sum() > ball.sum() and back.sum() < grown.sum()
    assert np.all(back[ball == 1] == 1)
    assert np.array_equal(mask_ref.extend(ball, 0.0), ball)


def test_both_loop_orders_of_the_scatter_agree(monkeypatch):
    """the restatement picks the cheaper loop order; both visit the same
    (source, offset) set, faces included"""
    rng = np.random.default_rng(1)
    m = (rng.random((N, N, N)) < 0.05).astype(np.float32)
    m[N // 2 - 1] = 1                                   # a slab on the positive k face
    out = {}
    for order in ("offsets", "sources"):
        monkeypatch.setattr(mask_ref, "FORCE_ORDER", order)
        out[order] = [mask_ref.extend(m, 2.5), mask_ref.extend(m, -2.0), mask_ref.soft_edge(m, 3.5)]
    for x, y in zip(out["offsets"], out["sources"]):
        assert np.array_equal(x, y)


def test_isolated_voxel_on_a_face_goes_and_a_face_pair_stays():
    h = N // 2
    src = np.zeros((N, N, N), np.float32)
    src[0, 0, (-h) % N] = 1                 # alone on the negative i face; its wrapped
    src[0, 0, h - 1] = 1                    # neighbour is on the positive face: both isolated
    src[3, (-h) % N, 2] = 1                 # a pair along k on the negative j face
    src[4, (-h) % N, 2] = 1
    got = mask_ref.threshold(src, 0.5, remove_corners=False)
    assert got[0, 0, (-h) % N] == 0 and got[0, 0, h - 1] == 0
    assert got[3, (-h) % N, 2] == 1 and got[4, (-h) % N, 2] == 1
    assert got.sum() == 2
    # corners count as 0 before the threshold
    full = np.ones((N, N, N), np.float32)
    k, j, i = signed_grid(N)
    assert np.array_equal(mask_ref.threshold(full, 0.5) == 1, i * i + j * j + k * k < h * h)
