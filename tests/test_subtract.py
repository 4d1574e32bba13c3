"""Signal subtraction without a GPU: the entry points of csrc/subtract.hip
reject bad arguments on the host, the restatement of tests/subtract_ref.py keeps
the reference's sign and axis conventions (pinned independently of the kernel),
and the host writer of thunder_amd/subtract.py lays the stack and the .thu
table out as saveSubtract / saveDatabase do (src/Optimiser.cpp:8418-8537,
8287-8360)."""
import ctypes

import numpy as np
import pytest

import subtract_ref
from thunder_amd import _lib, build, io, synth

PF = 2


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def _subtract_args(idim=32, r=15, nSym=0, symR=None, outs=True, diffRL=None, ws=None, wsBytes=0,
                   nImg=4, vdim=64):
    p = ctypes.c_void_p(16)
    o = p if outs else None
    return (p, vdim, PF, 1, p, p, p, p, None, None, None, nImg, idim, r, symR, nSym, None, o, None,
            diffRL, 1, o, o, ws, ctypes.c_size_t(wsBytes), None)


def test_entry_points_validate_without_gpu(L):
    p = ctypes.c_void_p(16)
    ok, bad = 0, 1
    assert L.thx_subtract(*_subtract_args(r=0)) == bad
    assert L.thx_subtract(*_subtract_args(r=16)) == bad          # idim/2 - 1 = 15 is the last
    assert b"r=16" in L.thx_last_error()
    assert L.thx_subtract(*_subtract_args(idim=31, r=10)) == bad
    assert b"even" in L.thx_last_error()
    assert L.thx_subtract(*_subtract_args(nSym=-1)) == bad
    assert L.thx_subtract(*_subtract_args(outs=False)) == bad
    assert b"output" in L.thx_last_error()
    assert L.thx_subtract(*_subtract_args(nSym=3, symR=None)) == bad
    assert b"symR" in L.thx_last_error()
    need = L.thx_subtract_workspace(4, 32, 3, 1)
    assert L.thx_subtract(*_subtract_args(nSym=3, symR=p, diffRL=p, ws=p, wsBytes=need - 1)) == bad
    assert b"workspace" in L.thx_last_error()
    assert L.thx_subtract(*_subtract_args(nSym=3, symR=p, diffRL=p, ws=None, wsBytes=need)) == bad
    assert L.thx_subtract(*_subtract_args(vdim=48)) == bad       # r * pf reaches the edge
    assert L.thx_subtract(*_subtract_args(nImg=0)) == ok         # an empty batch is a no-op
    assert L.thx_region_centroid(p, 15, p, p, 1 << 20, None) == bad
    assert L.thx_region_centroid(None, 16, p, p, 1 << 20, None) == bad
    assert L.thx_region_centroid(p, 16, p, p, 8, None) == bad
    assert b"workspace" in L.thx_last_error()


def test_workspace_queries_are_host_only(L):
    per = 32 * 17 * 8
    assert L.thx_subtract_workspace(7, 32, 0, 0) == 0
    assert L.thx_subtract_workspace(7, 32, 0, 1) >= 7 * per
    assert L.thx_subtract_workspace(7, 32, 59, 1) >= 60 * 7 * per
    assert L.thx_subtract_workspace(7, 31, 0, 1) == 0
    assert L.thx_subtract_workspace(7, 32, -1, 1) == 0
    assert L.thx_region_centroid_workspace(16) >= 4 * 8
    assert L.thx_region_centroid_workspace(15) == 0
    # the partial sums of at most 1024 blocks, whatever the box
    assert L.thx_region_centroid_workspace(512) <= 4 * 1024 * 8 + 256


def _image_stack(n, N, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((n, N, N))
    return img, np.fft.rfft2(img).astype(np.complex128)


def test_restatement_zero_model_is_a_roll(orc):
    """no model, the identity pose, -t + offS - centre = (3, -2): the output is
    the input image moved by (3, -2) pixels, x along columns"""
    N, r, n = 16, 7, 2
    img, ft = _image_stack(n, N, 1)
    vols = np.zeros((1, N * PF, N * PF, N * PF // 2 + 1), np.complex64)
    quat = np.tile([1.0, 0, 0, 0], (n, 1))
    centre = np.array([-1.0, 0.5, 2.0])
    off = np.tile([0.25, -1.0], (n, 1))
    trans = off - centre[:2] - np.array([3.0, -2.0])
    o = subtract_ref.subtract(orc, vols, N * PF, PF, ft, synth.ctf_attrs(n, seed=2), quat, trans, r,
                              N, offS=off, centre=centre)
    want = np.roll(img, (-2, 3), axis=(1, 2))
    assert np.max(np.abs(o.diffRL[0] - want)) <= 1e-12 * np.abs(img).max()
    assert np.array_equal(o.shift, trans - off)
    assert np.max(np.abs(subtract_ref.centred(o.diffRL[0])
                         - np.roll(np.fft.fftshift(img, axes=(1, 2)), (-2, 3), axis=(1, 2)))) <= 1e-12 * np.abs(img).max()


def test_restatement_copy_is_copy0_of_the_symmetric_pose(orc):
    """copy s = copy 0 of a call posed at symR[s-1]^T rotB.  The second call
    reaches the matrix through a quaternion (1e-15), so the oracle's FP32
    coordinates may round the other way: 1e-5 of the image, the project's
    tolerance"""
    from thunder_amd import ops
    N, r, n = 16, 7, 3
    _, ft = _image_stack(n, N, 3)
    vols = np.stack([synth.projectee(synth.blob_volume(N, n_blobs=10, seed=5), PF).numpy()])
    rng = np.random.default_rng(4)
    quat = synth.uniform_quaternions(n, rng)
    trans = rng.standard_normal((n, 2))
    attr = synth.ctf_attrs(n, seed=6)
    symR, _ = ops.symmetry("D2")
    centre = np.array([1.5, -2.0, 0.75])
    o = subtract_ref.subtract(orc, vols, N * PF, PF, ft, attr, quat, trans, r, N, symR=symR,
                              centre=centre)
    assert o.diffFT.shape[0] == 4
    scale = np.abs(ft).max()
    for s in range(1, 4):
        q = np.stack([subtract_ref.quaternion(symR[s - 1].T @ subtract_ref.rot_matrix(orc, quat[l]))
                      for l in range(n)])
        assert np.allclose(q, o.quat[s], atol=1e-14)
        one = subtract_ref.subtract(orc, vols, N * PF, PF, ft, attr, q, trans, r, N, centre=centre)
        assert np.max(np.abs(one.diffFT[0] - o.diffFT[s])) <= 1e-5 * scale
        assert np.max(np.abs(one.modelFT[0] - o.modelFT[s])) <= 1e-5 * scale
        assert np.abs(o.modelFT[s]).max() > 1e-3 * scale        # there is a model to compare
        for l in range(n):
            assert np.allclose(subtract_ref.quat_matrix(o.quat[s, l]),
                               symR[s - 1].T @ subtract_ref.rot_matrix(orc, quat[l]), atol=1e-12)


def soft_mask(N, c, rad, edge=3.0):
    """an off-centre soft mask [k][j][i], origin at index 0"""
    co = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(np.float64)
    k, j, i = np.meshgrid(co, co, co, indexing="ij")
    d = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2)
    return np.exp(-np.maximum(d - rad, 0) ** 2 / (2 * edge ** 2)).astype(np.float32)


def test_restatement_centroid():
    N = 16
    c = (2.0, -1.5, 3.0)
    m = soft_mask(N, c, 2.0, 1.2)
    got = subtract_ref.region_centroid(m)
    sh = np.fft.fftshift(m).astype(np.float64)
    ax = np.arange(-N // 2, N // 2, dtype=np.float64)
    direct = np.array([np.einsum("kji,i->", sh, ax), np.einsum("kji,j->", sh, ax),
                       np.einsum("kji,k->", sh, ax)]) / sh.sum()
    assert np.allclose(got, direct, rtol=1e-12, atol=1e-13)
    assert np.allclose(got, c, atol=0.05)          # the mask sits where it was put


def test_writer_round_trip(tmp_path):
    from thunder_amd import subtract
    n, copies, N = 3, 2, 8
    rng = np.random.default_rng(7)
    rl = rng.standard_normal((copies, n, N, N)).astype(np.float32)
    quat = synth.uniform_quaternions(copies * n, rng).reshape(copies, n, 4)
    attr = synth.ctf_attrs(n, seed=8)
    group = np.array([2, 0, 1])
    cls = np.array([1, 0, 1], np.int32)
    prefix = str(tmp_path / "out") + "/"          # prepended as a string, like dstPrefix
    sp, tp = subtract.write_subtract(prefix, rl, quat, attr, group=group, cls=cls, rank=3,
                                     pixel_size=1.32)
    assert sp == prefix + "Subtract_Rank_000003.mrcs" and tp == prefix + "Meta_Subtract.thu"
    h, data = io.read_mrc(sp)
    assert (h.nz, h.ny, h.nx) == (copies * n, N, N)
    assert h.pixel_size == pytest.approx(1.32, rel=1e-6)
    assert np.array_equal(np.asarray(data), rl.reshape(-1, N, N))
    t = io.read_thu(tp)
    assert len(t["particlePath"]) == copies * n
    row = 0
    for l in range(n):                       # image outer, copy inner
        for s in range(copies):
            assert t["particlePath"][row] == "%012d@Subtract_Rank_000003.mrcs" % (l + n * s + 1)
            idx = int(t["particlePath"][row].split("@")[0]) - 1
            assert np.array_equal(np.asarray(data[idx]), rl[s, l])
            q = np.array([t[f"quat{k}"][row] for k in range(4)])
            assert np.allclose(q, quat[s, l], atol=1e-9)          # %18.9f
            assert t["transX"][row] == 0 and t["transY"][row] == 0
            assert t["groupID"][row] == group[l] and t["classID"][row] == cls[l]
            assert t["voltage"][row] == pytest.approx(float(attr[l, 1]), rel=1e-6)
            assert t["defocusU"][row] == pytest.approx(float(attr[l, 2]), rel=1e-6)
            assert t["defocusFactor"][row] == 1.0
            row += 1
    # the table loads back as a stack of the written planes
    imgs = io.load_images(t, prefix=prefix)
    assert np.array_equal(imgs.reshape(n, copies, N, N), rl.transpose(1, 0, 2, 3))
