"""thx_step_compact_order (csrc/geom.hip): the tile order without its
all-padding steps, the visiting order of the box-less local-phase kernels.
A step is 4 aligned entries; the compaction removes the steps that are four
-1, keeps every other step as it is and in sequence, and pads the end with -1
to a multiple of 32 (one iteration of those kernels)."""
import ctypes

import numpy as np
import pytest

from thunder_amd import _lib, build, ops

# (box, rU): the bench's set, the two odd-group-count sets of the test configs,
# and a tiny set whose groups are mostly partial squares
SHAPES = [(64, 20), (200, 19), (256, 24), (32, 6)]


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def steps(o):
    return np.asarray(o).reshape(-1, 4)


@pytest.mark.parametrize("N,rU", SHAPES)
def test_compacted_order(L, N, rU):
    px = ops.PixelSet(N, 2, rU, 1)
    o = px.order
    c = ops.step_compact_order(o)
    # same pixels in the same sequence
    assert np.array_equal(c[c >= 0], o[o >= 0])
    assert len(c) % 32 == 0
    has = (steps(c) >= 0).any(axis=1)
    n_real = int(np.nonzero(has)[0][-1]) + 1
    # every step before the final padding holds a pixel; the padding is short
    assert has[:n_real].all()
    assert len(c) - 4 * n_real < 32
    assert (c[4 * n_real:] == -1).all()
    # every step of the input that holds a pixel appears unchanged, in sequence
    so = steps(o)
    kept = so[(so >= 0).any(axis=1)]
    assert np.array_equal(steps(c)[:n_real], kept)
    # the sets do have all-padding steps before their last pixel (what is removed)
    pad = np.nonzero(~(so >= 0).any(axis=1))[0]
    assert len(pad) > 0 and pad[0] < np.nonzero((so >= 0).any(axis=1))[0][-1]
    # compacting twice is compacting once
    assert np.array_equal(ops.step_compact_order(c), c)


def test_bench_shape_counts(L):
    """Box 256, rU 24: 870 pixels in 944 entries (59 groups); 15 all-padding
    steps leave 221, 224 after rounding to whole 8-step iterations."""
    px = ops.PixelSet(256, 2, 24, 1)
    assert (px.n, len(px.order)) == (870, 944)
    assert int((~(steps(px.order) >= 0).any(axis=1)).sum()) == 15
    assert len(ops.step_compact_order(px.order)) == 896
    # the sets of the GPU bit-identity tests: odd group count / mostly partial groups
    assert (len(ops.PixelSet(64, 2, 20, 1).order) // 16) % 2 == 1


def test_compaction_arguments(L):
    vp = ctypes.c_void_p
    n = ctypes.c_int(-1)
    o = np.array([-1, -1, -1, -1, 3, -1, -1, -1], np.int32)
    # size query, then a cap that is too small
    assert L.thx_step_compact_order(o.ctypes.data_as(vp), 8, 0, None, ctypes.byref(n)) == 0
    assert n.value == 32
    out = np.zeros(32, np.int32)
    assert L.thx_step_compact_order(o.ctypes.data_as(vp), 8, 16, out.ctypes.data_as(vp),
                                    ctypes.byref(n)) == 1
    assert L.thx_step_compact_order(o.ctypes.data_as(vp), 8, 32, out.ctypes.data_as(vp),
                                    ctypes.byref(n)) == 0
    assert out.tolist() == [3, -1, -1, -1] + [-1] * 28
    # not whole steps; an empty order stays empty
    assert L.thx_step_compact_order(o.ctypes.data_as(vp), 6, 32, out.ctypes.data_as(vp),
                                    ctypes.byref(n)) == 1
    assert L.thx_step_compact_order(None, 0, 0, None, ctypes.byref(n)) == 0 and n.value == 0
