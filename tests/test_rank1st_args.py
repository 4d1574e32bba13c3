"""CPU-side checks of the rank1st reader and the between-round entry points
(csrc/optimiser.hip thx_expectation_rank1st, csrc/round.hip): the library
exposes them through _lib.py and each rejects bad arguments with THX_ERR_ARG
and a message before any device work; an empty batch is a no-op."""
import ctypes

import pytest

from thunder_amd import _lib, build
from thunder_amd.expectation import CtfSearchCfg, ExpectCfg

OK, BAD = 0, 1
d = ctypes.c_void_p(4096)
BIG = ctypes.c_size_t(1 << 40)
NEW = ("thx_expectation_rank1st", "thx_rank1st_diff", "thx_recentre", "thx_class_count")


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def local_cfg():
    # a local search at box 32, pf 2: 9 rotations x 9 translations, one phase
    return ExpectCfg(32, 2, 64, 0, 0, 9, 9, 1, 4, 0.5, 0.0, 0.0, 10.0, 60.0, 7, 1,
                     1, 1, 0, 3, 100, 1, 100, 2.0, 0, None, None, 0, None, 0, None, 0)


def rejected(L, status):
    return status == BAD and len(L.thx_last_error()) > 0


def test_library_exposes_the_new_symbols(L):
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.thx_abi_version() == 9


def test_rank1st_reader_validates_without_gpu(L):
    cfg, cs = local_cfg(), CtfSearchCfg(9, 0.01, 0.5, None, None, None)
    nImg, nPxl = 5, 300

    def call(cfg=ctypes.byref(cfg), cs=None, n=nImg, ws=d, nb=BIG, q=d, t=d, dd=None, v=d):
        return L.thx_expectation_rank1st(cfg, cs, 0, n, nPxl, 0, ws, nb, q, t, dd, v, None)

    assert rejected(L, call(cfg=None)) and rejected(L, call(ws=None))
    assert rejected(L, call(n=-1))
    assert rejected(L, call(dd=d))                       # topD without a CTF search
    assert b"topD" in L.thx_last_error()
    assert rejected(L, call(q=None)) and rejected(L, call(t=None))
    need = L.thx_expectation_workspace(ctypes.byref(cfg), nImg, nPxl, 0)
    assert need > 0
    # (the query leaves room for any placement of the y-pair copy, so the
    # plan on a given buffer may be smaller than it: probe well below both)
    assert rejected(L, call(nb=ctypes.c_size_t(need // 64)))
    assert b"workspace" in L.thx_last_error()
    # a CTF search has a plan of its own
    cfg.searchType = 2
    need_d = L.thx_expectation_ctf_workspace(ctypes.byref(cfg), ctypes.byref(cs), nImg, nPxl, 0)
    assert need_d > 0
    assert rejected(L, call(cs=ctypes.byref(cs), dd=d, nb=ctypes.c_size_t(need_d // 64)))
    assert b"workspace" in L.thx_last_error()
    # an empty batch: nothing to copy, whatever the pointers
    assert call(n=0, q=None, t=None, v=None) == OK
    assert call(n=0, cs=ctypes.byref(cs), dd=None) == OK


def test_rank1st_diff_validates_without_gpu(L):
    def call(n=4, q=(d, d, d), t=(d, d, d), dd=(None, None, None), c=(d, d, d)):
        return L.thx_rank1st_diff(n, *q, *t, *dd, *c, None)

    assert rejected(L, call(n=-1))
    for part in ((d, None, d), (d, d, None), (None, d, d)):   # a group given in part
        assert rejected(L, call(q=part)) and rejected(L, call(t=part))
        assert rejected(L, call(dd=part)) and rejected(L, call(c=part))
    assert call(n=0) == OK
    none = (None, None, None)
    assert call(q=none, t=none, c=none) == OK            # no group: nothing to do


def test_recentre_validates_without_gpu(L):
    def call(n=3, idim=32, ori=d, img=ctypes.c_void_p(1 << 30), top=d, off=d, mLT=9, tr=d, pt=d):
        return L.thx_recentre(n, idim, ori, img, top, off, mLT, tr, pt, None)

    assert rejected(L, call(n=-1))
    assert rejected(L, call(top=None)) and rejected(L, call(off=None))
    for idim in (0, -4, 31, 8194):
        assert rejected(L, call(idim=idim))
    assert b"idim" in L.thx_last_error()
    assert rejected(L, call(ori=None))                   # an image pass without its source
    assert rejected(L, call(img=d))                      # not in place
    assert rejected(L, call(mLT=0))
    assert call(n=0) == OK
    assert call(n=0, top=None, off=None, img=None, tr=None, pt=None) == OK


def test_class_count_validates_without_gpu(L):
    assert rejected(L, L.thx_class_count(-1, d, 4, d, None))
    assert rejected(L, L.thx_class_count(5, d, 0, d, None))
    assert rejected(L, L.thx_class_count(5, None, 4, d, None))
    assert rejected(L, L.thx_class_count(5, d, 4, None, None))
    assert L.thx_class_count(0, None, 4, None, None) == OK
