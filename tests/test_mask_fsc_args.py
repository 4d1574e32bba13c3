"""CPU-side checks of the mask-generation and masked-FSC entry points
(csrc/mask.hip, csrc/fsc_masked.hip): every one rejects bad arguments before
any device work, and the workspace queries are host-only.  Also the host
helper resolution.res_p against the restatement's."""
import ctypes

import numpy as np
import pytest

import fsc_masked_ref
from thunder_amd import _lib, build

OK, BAD = 0, 1
d = ctypes.c_void_p(4096)
d2 = ctypes.c_void_p(1 << 40)       # far from d: the maps do not overlap
BIG = ctypes.c_size_t(1 << 40)


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def test_mask_entry_points_validate_without_gpu(L):
    thr = lambda N=32, src=d, dst=d2: L.thx_mask_threshold(src, N, 0.5, 1, dst, None)
    ext = lambda N=32, e=2.5, src=d, dst=d2, ws=d, n=BIG: L.thx_mask_extend(src, N, e, dst, ws, n,
                                                                              None)
    soft = lambda N=32, e=6.0, src=d, dst=d2, ws=d, n=BIG: L.thx_mask_soft_edge(src, N, e, dst, ws,
                                                                                n, None)
    gen = lambda N=32, e=4.0, w=6.0, src=d, dst=d2, ws=d, n=BIG: L.thx_gen_mask(
        src, N, 0.5, e, w, 1, dst, ws, n, None)
    for f in (thr, ext, soft, gen):
        for N in (31, 33, 14, 0, -2, 1026, 2048):        # odd, out of [16, 1024]
            assert f(N=N) == BAD, N
        assert b"N=" in L.thx_last_error()
        assert f(src=None) == BAD and f(dst=None) == BAD
    assert thr(dst=d) == BAD and gen(dst=d) == BAD        # these two are not in place
    # |ext| and ew above 32
    assert ext(e=32.5) == BAD and ext(e=-33.0) == BAD and ext(e=float("nan")) == BAD
    assert b"ext" in L.thx_last_error()
    assert soft(e=32.25) == BAD and soft(e=float("nan")) == BAD
    assert b"ew" in L.thx_last_error()
    assert gen(e=40.0) == BAD and gen(e=-40.0) == BAD and gen(w=33.0) == BAD
    # a short or missing workspace
    need = L.thx_gen_mask_workspace(32)
    for f in (ext, soft, gen):
        assert f(n=ctypes.c_size_t(need - 1)) == BAD
        assert b"workspace" in L.thx_last_error()
        assert f(ws=None) == BAD


def test_fsc_masked_validates_without_gpu(L):
    call = lambda N=32, nShell=15, alpha=d, coreR=0.0, edge=6.0, method=0, A=d, B=d, fsc=d, ws=d, \
        n=BIG: L.thx_fsc_masked(A, B, N, nShell, alpha, coreR, edge, 1, method, fsc, None, None, ws,
                                n, None)
    for N in (31, 14, 0, 1026):
        assert call(N=N, nShell=5) == BAD
    assert b"N=" in L.thx_last_error()
    for ns in (0, 1, 17, -3):                            # outside [2, N/2]
        assert call(nShell=ns) == BAD
    assert b"nShell" in L.thx_last_error()
    # both masks, or neither
    assert call(alpha=d, coreR=8.0) == BAD
    assert b"exclusive" in L.thx_last_error()
    assert call(alpha=None, coreR=0.0) == BAD and call(alpha=None, coreR=-1.0) == BAD
    assert b"neither" in L.thx_last_error()
    assert call(alpha=None, coreR=8.0, edge=0.0) == BAD
    assert call(alpha=None, coreR=float("nan")) == BAD
    assert call(method=3) == BAD and call(method=-1) == BAD
    assert call(N=48, nShell=23, method=2) == BAD        # the column passes: powers of two
    assert call(A=None) == BAD and call(B=None) == BAD and call(fsc=None) == BAD
    need = L.thx_fsc_masked_workspace(32, 15)
    assert call(n=ctypes.c_size_t(need - 1)) == BAD
    assert b"workspace" in L.thx_last_error()
    assert call(ws=None) == BAD


def test_mask_fsc_workspace_queries_are_host_only(L):
    for N in (15, 33, 14, 0, 1026):
        assert L.thx_gen_mask_workspace(N) == 0
        assert L.thx_fsc_masked_workspace(N, 5) == 0
    assert L.thx_fsc_masked_workspace(32, 1) == 0 and L.thx_fsc_masked_workspace(32, 17) == 0
    # the packed bits: N^2 rows of ceil(N / 64) 64-bit words
    for N, words in ((32, 1), (64, 1), (96, 2), (512, 8)):
        assert L.thx_gen_mask_workspace(N) >= N * N * words * 8
        assert L.thx_gen_mask_workspace(N) < N * N * words * 8 + 4096
    # two half-complex copies and one real map at least
    N = 256
    assert L.thx_fsc_masked_workspace(N, 127) >= 2 * N * N * (N // 2 + 1) * 8 + N ** 3 * 4


def test_res_p_matches_the_restatement():
    from thunder_amd import resolution
    rng = np.random.default_rng(3)
    for _ in range(20):
        f = np.sort(rng.random(24))[::-1].copy()
        f[rng.integers(1, 24)] -= 0.3
        assert resolution.res_p(f, 0.8) == fsc_masked_ref.res_p(f, 0.8)
    ones = np.ones(15)
    assert resolution.res_p(ones, 0.8) == 14              # never below: the last shell
    assert resolution.res_p(np.zeros(15), 0.8) == 0       # shell 1 already below
    f = np.array([1.0, 0.9, 0.5, 0.2, 0.16, 0.1])
    assert resolution.res_p(f, 0.143, inverse=True) == 4
    assert resolution.res_p(f, 0.5) == 2 and resolution.res_p(f, 0.5, pf=2) == 1
