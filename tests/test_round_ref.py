"""The restatements of tests/round_ref.py against hand-computed values and
their own invariants, and thunder_amd.round.stat_mas against them (CPU)."""
import numpy as np
import pytest
import torch

import round_ref
from thunder_amd import round as rnd


@pytest.mark.parametrize("x, med, mad", [
    ([3.0], 3.0, 0.0),
    ([4.0, 1.0], 2.5, 1.5),                  # |x - 2.5| = 1.5, 1.5
    ([9.0, 1.0, 2.0], 2.0, 1.0),             # |x - 2| = 0, 1, 7
    ([1.0, 2.0, 4.0, 8.0], 3.0, 1.5),        # |x - 3| = 1, 1, 2, 5 -> 1.5
    ([2.0, 2.0, 2.0, 5.0, 5.0, 7.0], 3.5, 1.5),   # ties: |x - 3.5| = 1.5 x 5, 3.5
])
def test_stat_mas_hand_computed(x, med, mad):
    for f in (round_ref.stat_mas, rnd.stat_mas, lambda v: rnd.stat_mas(torch.tensor(v))):
        m, s = f(x)
        assert m == med and s == mad * 1.4826


def test_stat_mas_matches_the_restatement_on_random_sets():
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 64, 257):
        x = rng.standard_normal(n)
        assert rnd.stat_mas(torch.from_numpy(x)) == pytest.approx(round_ref.stat_mas(x), rel=1e-15)


def test_diff_top_sign_and_equality():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((6, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cur = {"quat": -q, "trans": np.ones((6, 2)), "d": np.full(6, 1.25),
           "cls": np.array([0, 1, 2, 0, 1, 2], np.int32)}
    prev = {"quat": q, "trans": np.ones((6, 2)) + [3.0, 4.0], "d": np.full(6, 1.0),
            "cls": np.array([0, 1, 0, 0, 2, 2], np.int32)}
    out, new = round_ref.diff_top(cur, prev)
    assert np.max(np.abs(out["diffR"])) < 4e-16          # q and -q are one rotation
    assert np.all(out["diffT"] == 5.0) and np.all(out["diffD"] == 0.25)
    assert out["sameC"].tolist() == [1, 1, 0, 1, 0, 1]   # equality, not difference
    for k in cur:
        assert np.array_equal(new[k], cur[k])


def test_recentre_there_and_back_restores_the_offset():
    rng = np.random.default_rng(2)
    off = rng.integers(-8, 8, (5, 2)) * 0.25             # exact in binary
    t = rng.integers(-8, 8, (5, 2)) * 0.125
    a = round_ref.recentre(None, t, off)
    b = round_ref.recentre(None, -t, a["off"])
    assert np.array_equal(b["off"], off)


@pytest.mark.parametrize("fp32", [False, True])
def test_recentre_integer_shift_is_a_roll(fp32):
    rng = np.random.default_rng(3)
    N = 16
    img = rng.standard_normal((2, N, N))
    ori = np.fft.rfft2(img)
    t = np.array([[3.0, -5.0], [-2.0, 7.0]])             # (x = column, y = row)
    out = round_ref.recentre(ori, t, np.zeros((2, 2)), fp32=fp32)
    # offS = -t; translate() by (ox, oy) moves the image by +ox columns, +oy rows
    back = np.fft.irfft2(out["img"], s=(N, N))
    for l in range(2):
        want = np.roll(img[l], (int(-t[l, 1]), int(-t[l, 0])), axis=(0, 1))
        assert np.max(np.abs(back[l] - want)) < (1e-5 if fp32 else 1e-12)


def test_recentre_moves_the_whole_state_by_t():
    rng = np.random.default_rng(4)
    t = rng.standard_normal((7, 2))
    trans, prev, off = rng.standard_normal((7, 9, 2)), rng.standard_normal((7, 2)), \
        rng.standard_normal((7, 2))
    out = round_ref.recentre(None, t, off, trans, prev)
    assert np.array_equal(out["trans"], trans - t[:, None])
    assert np.array_equal(out["prev_t"], prev - t)
    assert np.array_equal(out["off"], off - t)
    assert np.all(out["top_t"] == 0.0)


def test_class_count_accumulates_and_skips_out_of_range():
    c = round_ref.class_count([0, 2, 2, 5, -1, 3], 4)
    assert c.tolist() == [1, 0, 2, 1]
    assert round_ref.class_count([1, 1], 4, c).tolist() == [1, 2, 2, 1]
