"""CPU-side checks of the map tools (csrc/maptools.hip, thunder_amd/maptools.py): every entry
point rejects bad arguments with THX_ERR_ARG and a message before any device work, the workspace
queries are host-only, and an empty batch is accepted without a launch.  The transform's nMat = 0
is a launch (a copy or a clear) and runs in tests/test_gpu_maptools.py; here its arguments are
shown to pass the checks by being refused only for the one thing that is wrong."""
import ctypes

import numpy as np
import pytest
import torch

from thunder_amd import _lib, build, maptools

OK, BAD = 0, 1
d, e = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
NEW = ("thx_vol_transform_rl", "thx_ft_resize", "thx_vol_resize_workspace", "thx_vol_resize",
       "thx_project_images_workspace", "thx_project_images", "thx_vol_soft_mask")


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def rejected(L, status, word=None):
    msg = L.thx_last_error()
    return status == BAD and len(msg) > 0 and (word is None or word.encode() in msg)


def test_library_exposes_the_new_symbols(L):
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.thx_abi_version() == 9


def test_transform_validates_without_gpu(L):
    def call(src=d, N=16, mat=d, nMat=1, r=7.0, interp=1, add=0, dst=e):
        return L.thx_vol_transform_rl(src, N, mat, nMat, r, interp, add, dst, None)

    for N in (0, 14, 17, 1026, -16):
        assert rejected(L, call(N=N), "N="), N
    assert rejected(L, call(nMat=-1), "nMat")
    for r in (0.0, -1.0, 7.5, 8.0, float("nan"), float("inf")):     # (0, N/2 - 1] only
        assert rejected(L, call(r=r), "r="), r
    for interp in (-1, 2):
        assert rejected(L, call(interp=interp), "interp")
    assert rejected(L, call(dst=d), "dst must not be src")
    assert rejected(L, call(src=None), "NULL") and rejected(L, call(dst=None), "NULL")
    assert rejected(L, call(mat=None), "mat is NULL")
    # nMat = 0 needs no matrices: only the remaining fault is reported
    assert rejected(L, call(mat=None, nMat=0, r=0.0), "r=")
    assert rejected(L, call(mat=None, nMat=0, dst=d), "dst must not be src")


def test_resize_validates_without_gpu(L):
    for N, M in ((14, 16), (16, 14), (17, 16), (16, 2048), (0, 16)):
        assert rejected(L, L.thx_ft_resize(d, N, e, M, None)), (N, M)
        assert rejected(L, L.thx_vol_resize(d, N, e, M, d, 1 << 40, None)), (N, M)
        assert L.thx_vol_resize_workspace(N, M) == 0
    assert rejected(L, L.thx_ft_resize(None, 16, e, 32, None), "NULL")
    assert rejected(L, L.thx_ft_resize(d, 16, None, 32, None), "NULL")
    assert rejected(L, L.thx_ft_resize(d, 16, d, 32, None), "must not be")
    need = L.thx_vol_resize_workspace(16, 32)
    # the real copy, both transforms and hipFFT's reserve at the larger box
    assert need >= 4 * 16 ** 3 + 8 * (9 * 16 * 16 + 17 * 32 * 32) + 2 * 8 * 17 * 32 * 32
    assert rejected(L, L.thx_vol_resize(None, 16, e, 32, d, need, None), "NULL")
    assert rejected(L, L.thx_vol_resize(d, 16, None, 32, d, need, None), "NULL")
    assert rejected(L, L.thx_vol_resize(d, 16, e, 32, None, need, None), "workspace")
    assert rejected(L, L.thx_vol_resize(d, 16, e, 32, d, need - 1, None), "workspace")


def test_project_validates_without_gpu(L):
    big = 1 << 40

    def call(vol=d, vdim=32, pf=2, mat=d, trans=None, n=3, N=16, r=7, ft=e, rl=e, centred=0, ws=d,
             nbytes=big):
        return L.thx_project_images(vol, vdim, pf, mat, trans, n, N, r, ft, rl, centred, ws, nbytes,
                                    None)

    for N in (14, 17, 0):
        assert rejected(L, call(N=N, vdim=2 * N), "N="), N
    assert rejected(L, call(vdim=48), "vdim") and rejected(L, call(pf=0), "vdim")
    assert rejected(L, call(n=-1), "n=")
    for r in (0, 8, -3):
        assert rejected(L, call(r=r), "r="), r
    assert rejected(L, call(ft=None, rl=None), "both NULL")
    assert rejected(L, call(vol=None), "NULL") and rejected(L, call(mat=None), "NULL")
    need = L.thx_project_images_workspace(3, 16)
    assert need >= 3 * 16 * 9 * 8
    assert rejected(L, call(ws=None), "workspace") and rejected(L, call(nbytes=need - 1), "workspace")
    assert rejected(L, call(ft=None, ws=None), "workspace")          # imgRL needs it
    assert L.thx_project_images_workspace(-1, 16) == 0 and L.thx_project_images_workspace(3, 15) == 0
    assert L.thx_project_images_workspace(0, 16) > 0
    # an empty batch: THX_OK without a launch, whatever the pointers; the sizes are checked even then
    assert call(n=0) == OK
    assert call(n=0, vol=None, mat=None, rl=None, ws=None, nbytes=0) == OK
    assert rejected(L, call(n=0, r=0), "r=")


def test_soft_mask_validates_without_gpu(L):
    assert rejected(L, L.thx_vol_soft_mask(d, 19, 5.0, 6.0, d, None), "N=")
    for r, ew in ((-1.0, 6.0), (float("nan"), 6.0), (5.0, 0.0), (5.0, -2.0), (5.0, float("inf"))):
        assert rejected(L, L.thx_vol_soft_mask(d, 16, r, ew, d, None)), (r, ew)
    assert rejected(L, L.thx_vol_soft_mask(None, 16, 5.0, 6.0, d, None), "NULL")
    assert rejected(L, L.thx_vol_soft_mask(d, 16, 5.0, 6.0, None, None), "NULL")


def test_python_front_end_refuses_before_the_library():
    """shapes, dtypes and devices are checked on the host tensors"""
    v = torch.zeros(16, 16, 16)
    with pytest.raises(ValueError, match="device"):
        maptools.transform(v, np.eye(3)[None])
    with pytest.raises(ValueError, match=r"expected \[N, N, N\]"):
        maptools.soft_mask(torch.zeros(16, 16, 8), 5)
    with pytest.raises(ValueError, match="even"):
        maptools.resize(v, 15)
    with pytest.raises(ValueError, match="half-complex"):
        maptools.ft_resize(torch.zeros(16, 16, 16, dtype=torch.complex64), 32)
    with pytest.raises(ValueError, match="non-zero"):
        maptools.align_z(v, (0, 0, 0))
    with pytest.raises(ValueError, match="rank"):
        maptools.run_project("in.mrc", "out", "meta.txt", 4, 1.0, 1, rank=2, world=2)
