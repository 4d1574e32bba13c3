"""Mask generation on the GPU (csrc/mask.hip, thunder_amd/mask.py) against the
scatter-form restatement of tests/mask_ref.py (src/Functions/Mask.cpp:581-731).

Boxes: 32 (narrower than one 64-bit word of the packed rows), 64 (exactly one
word), 96 (a word and a half, not a power of two).  Inputs: a blob volume
thresholded at its 90th percentile, a random field of density 0.5 % (isolated
points), and slabs on the three negative and the three positive faces (the
box-face rule; thresholded without the corner removal, which would clear the
faces).

threshold and extend are bit-exact.  The soft edge changes exactly the same set
of voxels and its values agree within 1e-6 absolute: FP32 cosf is good to a
couple of ulps and its argument d / ew pi carries at most a few ulps of pi,
about 7e-7, with |d cos| <= 1 and a factor 0.5 in front.
"""
import numpy as np
import pytest
import torch

import mask_ref
from thunder_amd import mask, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BOXES = [32, 64, 96]
INPUTS = ["blob", "sparse", "slab"]
EXTS = [0.0, 1.0, 2.5, 4.0, -2.0, -2.5]
EDGES = [0.0, 1.0, 3.5, 6.0]
SOFT_TOL = 1e-6


def T_(a):
    return torch.as_tensor(np.array(a, np.float32), device=DEV)


_src, _thr = {}, {}


def source(N, kind):
    """(map with the origin at index 0, threshold, remove_corners)"""
    key = (N, kind)
    if key not in _src:
        rng = np.random.default_rng(N + len(kind))
        if kind == "blob":
            v = np.fft.ifftshift(synth.blob_volume(N, n_blobs=30, seed=2).numpy())
            _src[key] = (v, float(np.percentile(v, 90)), True)
        elif kind == "sparse":
            v = (rng.random((N, N, N)) < 0.005).astype(np.float32)
            _src[key] = (v, 0.5, True)
        else:
            c = np.zeros((N, N, N), np.float32)            # centred: index p = i + N/2
            c[:2, 5:N - 9, 3:N - 4] = 1                    # the negative k, j, i faces
            c[4:N - 3, :2, 7:N - 5] = 1
            c[6:N - 7, 2:N - 6, :2] = 1
            c[-2:, 3:N - 8, 6:N - 3] = 1                   # the positive ones
            c[5:N - 2, -2:, 4:N - 9] = 1
            c[3:N - 6, 8:N - 4, -2:] = 1
            c[N // 2, N // 2, N // 2] = 1                  # an isolated point at the origin
            _src[key] = (np.fft.ifftshift(c), 0.5, False)
    return _src[key]


def thresholded(N, kind):
    key = (N, kind)
    if key not in _thr:
        v, t, rc = source(N, kind)
        _thr[key] = mask_ref.threshold(v, t, rc)
        _thr[key].setflags(write=False)
    return _thr[key]


def binary(N, kind):
    """the 0 / 1 map the later stages start from: the thresholded map, but the
    raw field for "sparse" (its isolated points are what that input is for)"""
    return source(N, kind)[0] if kind == "sparse" else thresholded(N, kind)


_ext = {}


def extended(N, kind, ext, m=None):
    key = (N, kind, ext, m is None)
    if key not in _ext:
        _ext[key] = mask_ref.extend(binary(N, kind) if m is None else m, ext)
        _ext[key].setflags(write=False)
    return _ext[key]


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("N", BOXES)
def test_threshold_is_bit_exact(N, kind):
    v, t, rc = source(N, kind)
    for corners in (rc, not rc):
        want = thresholded(N, kind) if corners == rc else mask_ref.threshold(v, t, corners)
        got = mask.threshold(T_(v), t, corners).cpu().numpy()
        assert np.array_equal(got, want), (N, kind, corners, int((got != want).sum()))
    if kind != "blob":
        assert (v > t).sum() > thresholded(N, kind).sum()      # isolated points were there


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("N", BOXES)
def test_extend_is_bit_exact(N, kind, ext):
    m = binary(N, kind)
    want = extended(N, kind, ext)
    got = mask.extend(T_(m), ext).cpu().numpy()
    assert np.array_equal(got, want), (N, kind, ext, int((got != want).sum()))
    if abs(ext) > 1:            # |d|^2 < 1 is the voxel itself
        assert not np.array_equal(want, m)


def check_soft(got, want, src, what):
    assert np.array_equal(got != src, want != src), (what, int(((got != src) != (want != src)).sum()))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: soft-edge max |gpu - ref| = {err:.3g} (bound {SOFT_TOL:g})")
    assert err <= SOFT_TOL, (what, err)


@pytest.mark.parametrize("ew", EDGES)
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("N", BOXES)
def test_soft_edge(N, kind, ew):
    m = binary(N, kind)
    want = mask_ref.soft_edge(m, ew)
    got = mask.soft_edge(T_(m), ew).cpu().numpy()
    check_soft(got, want, m, (N, kind, ew))
    if ew > 1:                  # 0 < |d| < 1 has no integer offset
        assert (want != m).any()


@pytest.mark.parametrize("kind", INPUTS)
def test_radius_32_reaches_the_whole_box(kind):
    """N = 32 with ext = 32 and ew = 32: the open ball's offsets go to +-31"""
    N = 32
    m = binary(N, kind)
    for ext in (32.0, -32.0):
        want = mask_ref.extend(m, ext)
        got = mask.extend(T_(m), ext).cpu().numpy()
        assert np.array_equal(got, want), (kind, ext)
    check_soft(mask.soft_edge(T_(m), 32.0).cpu().numpy(), mask_ref.soft_edge(m, 32.0), m,
               (N, kind, 32.0))
    one = np.zeros((N, N, N), np.float32)
    one[(-16) % N, (-16) % N, (-16) % N] = 1               # the corner voxel (-16, -16, -16)
    got = mask.extend(T_(one), 32.0).cpu().numpy()
    assert np.array_equal(got, mask_ref.extend(one, 32.0))
    assert got[16, 23, 15] == 1 and got[16, 24, 15] == 0    # d = (31, 7, 0): 1010; (31, 8, 0): 1025


@pytest.mark.parametrize("ext,ew", [(4.0, 6.0), (-2.0, 3.5), (2.5, 0.0)])
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("N", BOXES)
def test_gen_mask_is_the_three_stages_chained(N, kind, ext, ew):
    v, t, rc = source(N, kind)
    src = T_(v)
    chained = mask.soft_edge(mask.extend(mask.threshold(src, t, rc), ext), ew)
    got = mask.gen_mask(src, t, ext, ew, rc)
    assert torch.equal(got, chained)
    assert torch.equal(src, T_(v))                          # the input is untouched
    assert torch.equal(mask.gen_mask(src, t, ext, ew, rc), got)     # run to run
    stage2 = extended(N, kind, ext, thresholded(N, kind))
    check_soft(got.cpu().numpy(), mask_ref.soft_edge(stage2, ew), stage2, (N, kind, ext, ew))


@pytest.mark.parametrize("N", BOXES)
def test_two_runs_are_bitwise_equal(N):
    m = T_(thresholded(N, "blob"))
    for f, p in ((mask.extend, 2.5), (mask.extend, -2.5), (mask.soft_edge, 3.5)):
        assert torch.equal(f(m, p), f(m, p))


@pytest.mark.parametrize("N", BOXES)
def test_constant_maps_pass_the_soft_edge_unchanged(N):
    for value in (0.0, 1.0):
        m = torch.full((N, N, N), value, dtype=torch.float32, device=DEV)
        assert torch.equal(mask.soft_edge(m, 6.0), m)
        assert torch.equal(mask.extend(m, 2.5), m) and torch.equal(mask.extend(m, -2.5), m)


def test_a_soft_map_keeps_its_values_where_no_rule_applies():
    """voxels that are neither 0 nor 1 are no sources and are kept by extend"""
    N = 32
    m = np.array(thresholded(N, "blob"))
    soft = mask_ref.soft_edge(m, 3.5)
    for ext in (2.5, -2.5):
        assert np.array_equal(mask.extend(T_(soft), ext).cpu().numpy(), mask_ref.extend(soft, ext))
    # a second soft edge rewrites the edge voxels with the values they have, so the
    # changed sets are a matter of last bits here: values only
    got = mask.soft_edge(T_(soft), 3.5).cpu().numpy()
    assert float(np.abs(got - mask_ref.soft_edge(soft, 3.5)).max()) <= SOFT_TOL


def test_save_mask_writes_the_centred_layout(tmp_path):
    from thunder_amd import io
    N = 32
    v, t, rc = source(N, "blob")
    m = mask.gen_mask(T_(v), t, 2.0, 3.0, rc)
    path = mask.save_mask(str(tmp_path / "mask.mrc"), m, 1.32)
    _, data = io.read_mrc(path, mmap=False)
    assert np.array_equal(np.fft.ifftshift(np.asarray(data)), m.cpu().numpy())
