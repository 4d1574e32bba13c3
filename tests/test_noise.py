"""The host side of the noise model (csrc/noise.hip) without a GPU:
thx_spectrum_pixels against a brute-force walk of powerSpectrum's domain
(src/Functions/Spectrum.cpp:161-190), thx_sigma_finalise /
thx_sigma_init_finalise against the float64 restatement of
Optimiser::allReduceSigma's tail (src/Optimiser.cpp:6653-6708) and initSigma
(:5145-5243) on fabricated sums, and the argument validation of every device
entry point, which has to answer THX_ERR_ARG before anything is enqueued."""
import ctypes

import numpy as np
import pytest

import noise_ref
from thunder_amd import _lib, build

vp = ctypes.c_void_p
ERR_ARG = 1


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def P(a):
    return a.ctypes.data_as(vp)


def _table(L, N, r):
    n = ctypes.c_int(-1)
    start = np.full(r + 1, -1, np.int32)
    assert L.thx_spectrum_pixels(N, r, 0, None, None, None, None, P(start), ctypes.byref(n)) == 0
    bufs = [np.full(n.value, -7, np.int32) for _ in range(4)]
    m = ctypes.c_int(-1)
    assert L.thx_spectrum_pixels(N, r, n.value, *[P(b) for b in bufs], P(start),
                                 ctypes.byref(m)) == 0
    assert m.value == n.value
    return bufs, start


@pytest.mark.parametrize("N,r", [(32, 15), (32, 10), (64, 31), (200, 99)])
def test_spectrum_pixels_match_brute_force(L, N, r):
    (iCol, iRow, iShell, iPxl), start = _table(L, N, r)
    rc, rr, rs, rp, rstart = noise_ref.by_shell(N, r)
    assert np.array_equal(start, rstart)
    assert np.array_equal(iShell, rs)
    assert np.array_equal(iCol, rc) and np.array_equal(iRow, rr)
    assert np.array_equal(iPxl, rp)
    # the domain holds column 0 below the axis, which a1's pixel set skips
    assert np.any((iCol == 0) & (iRow < 0))
    assert len(np.unique(iPxl)) == len(iPxl) and iPxl.max() < N * (N // 2 + 1)


def test_spectrum_pixels_rejects_bad_radius(L):
    n = ctypes.c_int(0)
    for N, r in ((32, 16), (32, 0), (64, 32), (32, -3), (33, 4)):
        assert L.thx_spectrum_pixels(N, r, 0, None, None, None, None, None,
                                     ctypes.byref(n)) == ERR_ARG
    assert L.thx_spectrum_pixels(32, 15, 0, None, None, None, None, None, None) == ERR_ARG
    buf = np.zeros(4, np.int32)        # cap too small for the table
    assert L.thx_spectrum_pixels(32, 15, 4, P(buf), None, None, None, None,
                                 ctypes.byref(n)) == ERR_ARG


def _fabricated(n_group, r, seed):
    rng = np.random.default_rng(seed)
    acc = np.zeros((3, n_group, r + 1))
    cnt = rng.integers(1, 9, n_group).astype(np.float64)
    acc[:, :, r] = cnt
    acc[0, :, :r] = rng.uniform(0.5, 2.0, (n_group, r)) * cnt[:, None]
    acc[1, :, :r] = rng.uniform(1.0, 4.0, (n_group, r)) * cnt[:, None]
    acc[2, :, :r] = rng.uniform(0.2, 1.8, (n_group, r)) * cnt[:, None]   # both sides of min(1, .)
    return acc


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("n_group,r,n_col", [(3, 10, 16), (1, 15, 16), (4, 7, 12)])
def test_sigma_finalise_matches_restatement(L, grouped, n_group, r, n_col):
    acc = _fabricated(n_group, r, 11 + n_group)
    svd = acc[2, :, :r] / acc[2, :, r:]
    assert (svd > 1).any() and (svd < 1).any()
    alpha = 0.37
    sig = np.full((n_group, n_col), np.nan)
    rcp = np.full((n_group, n_col), np.nan)
    assert L.thx_sigma_finalise(P(acc), n_group, r, n_col, alpha, int(grouped), P(sig), P(rcp)) == 0
    rsig, rrcp = noise_ref.sigma_finalise(acc, n_col, alpha, grouped)
    assert np.allclose(sig, rsig, rtol=1e-12, atol=0)
    assert np.allclose(rcp, rrcp, rtol=1e-12, atol=0)
    if n_col - 1 > r:                   # the column extension ran
        assert np.array_equal(sig[:, r:n_col - 1], np.repeat(sig[:, r - 1:r], n_col - 1 - r, 1))
    if not grouped and n_group > 1:
        assert np.array_equal(sig[1:], np.repeat(sig[:1], n_group - 1, 0))


def test_sigma_finalise_rejects(L):
    acc = _fabricated(2, 10, 3)
    out = np.zeros((2, 16))
    assert L.thx_sigma_finalise(None, 2, 10, 16, 1.0, 1, P(out), P(out)) == ERR_ARG
    assert L.thx_sigma_finalise(P(acc), 2, 10, 16, 1.0, 1, None, P(out)) == ERR_ARG
    assert L.thx_sigma_finalise(P(acc), 2, 10, 10, 1.0, 1, P(out), P(out)) == ERR_ARG   # nCol < r+1
    assert L.thx_sigma_finalise(P(acc), 0, 10, 16, 1.0, 1, P(out), P(out)) == ERR_ARG


@pytest.mark.parametrize("N,r,n_group,n_col", [(32, 15, 3, 16), (32, 10, 2, 16), (64, 31, 1, 32)])
def test_sigma_init_finalise_matches_restatement(L, orc, N, r, n_group, n_col):
    rng = np.random.default_rng(N + r)
    n_total = 13.0
    avg = (rng.standard_normal((N, N // 2 + 1)) + 1j * rng.standard_normal((N, N // 2 + 1))) * 5 + 2
    ps = rng.uniform(40.0, 60.0, r) * n_total
    sig = np.full((n_group, n_col), np.nan)
    rcp = np.full((n_group, n_col), np.nan)
    a = np.ascontiguousarray(avg.astype(np.complex128)).view(np.float64)
    assert L.thx_sigma_init_finalise(P(a), P(ps), n_total, N, r, n_group, n_col, P(sig), P(rcp)) == 0
    px = noise_ref.disc(orc, N, r, 2)
    rsig, rrcp = noise_ref.init_finalise(avg, ps, n_total, px, r, n_group, n_col)
    assert np.allclose(sig, rsig, rtol=1e-12, atol=0)
    assert np.allclose(rcp, rrcp, rtol=1e-12, atol=0)
    assert L.thx_sigma_init_finalise(P(a), P(ps), n_total, N, N // 2, n_group, n_col + 8, P(sig),
                                     P(rcp)) == ERR_ARG
    assert L.thx_sigma_init_finalise(P(a), None, n_total, N, r, n_group, n_col, P(sig),
                                     P(rcp)) == ERR_ARG
    assert L.thx_sigma_init_finalise(P(a), P(ps), 0.0, N, r, n_group, n_col, P(sig),
                                     P(rcp)) == ERR_ARG


def test_device_entry_points_validate_before_launch(L):
    """NULLs, radii and shapes answer THX_ERR_ARG with no GPU present: nothing
    is enqueued.  `x` stands in for a device pointer; it is never dereferenced."""
    x = vp(0x1000)
    N, r, vdim, pf = 32, 15, 64, 2
    assert L.thx_power_spectrum(None, 1, N, r, x, x, x, None) == ERR_ARG
    assert L.thx_power_spectrum(x, 1, N, r, None, x, x, None) == ERR_ARG
    assert L.thx_power_spectrum(x, 1, N, r, x, x, None, None) == ERR_ARG
    assert L.thx_power_spectrum(x, 1, N, N // 2, x, x, x, None) == ERR_ARG
    assert L.thx_power_spectrum(x, -1, N, r, x, x, x, None) == ERR_ARG
    for fn in (L.thx_residual_spectra, L.thx_residual_spectra2d):
        def call(vol=x, vdim=vdim, pf=pf, nK=1, img=x, attr=x, rot=x, trans=x, n=1, N=N, r=r,
                 iCol=x, iShellStart=x, spectra=x, norm=None, rL=0.0, rN=0.0):
            return fn(vol, vdim, pf, nK, img, None, attr, rot, trans, None, None, None, n, N, r,
                      iCol, x, x, iShellStart, spectra, norm, rL, rN, None)
        for bad in (dict(vol=None), dict(img=None), dict(attr=None), dict(rot=None),
                    dict(trans=None), dict(iCol=None), dict(iShellStart=None), dict(spectra=None),
                    dict(r=0), dict(r=N // 2), dict(N=33), dict(nK=0), dict(n=-1), dict(pf=0),
                    dict(vdim=63), dict(vdim=32),            # r * pf reaches the volume edge
                    dict(norm=x, rL=2.0, rN=15.0),           # rNorm > r - 1/2
                    dict(norm=x, rL=5.0, rN=4.0), dict(norm=x, rL=-1.0, rN=4.0)):
            assert call(**bad) == ERR_ARG, bad
    assert L.thx_sigma_accumulate(None, None, 1, r, 1, x, None) == ERR_ARG
    assert L.thx_sigma_accumulate(x, None, 1, r, 1, None, None) == ERR_ARG
    assert L.thx_sigma_accumulate(x, None, 1, 0, 1, x, None) == ERR_ARG
    assert L.thx_sigma_accumulate(x, None, 1, r, 0, x, None) == ERR_ARG
    assert L.thx_sigma_accumulate(x, None, -1, r, 1, x, None) == ERR_ARG
    assert L.thx_sigma_init_accumulate(None, 1, N, r, x, x, x, x, None) == ERR_ARG
    assert L.thx_sigma_init_accumulate(x, 1, N, r, x, x, None, x, None) == ERR_ARG
    assert L.thx_sigma_init_accumulate(x, 1, N, r, x, x, x, None, None) == ERR_ARG
    assert L.thx_sigma_init_accumulate(x, 1, N, r, None, x, x, x, None) == ERR_ARG
    assert L.thx_sigma_init_accumulate(x, 1, N, N // 2, x, x, x, x, None) == ERR_ARG
    assert L.thx_sig_rcp_rows(None, 1, 16, None, x, 8, 1, x, None) == ERR_ARG
    assert L.thx_sig_rcp_rows(x, 1, 16, None, None, 8, 1, x, None) == ERR_ARG
    assert L.thx_sig_rcp_rows(x, 1, 16, None, x, 8, 1, None, None) == ERR_ARG
    assert L.thx_sig_rcp_rows(x, 0, 16, None, x, 8, 1, x, None) == ERR_ARG
    assert L.thx_sig_rcp_rows(x, 1, 16, None, x, 8, 70000, x, None) == ERR_ARG
    assert L.thx_img_scale(None, None, x, 1, N, None) == ERR_ARG
    assert L.thx_img_scale(x, None, None, 1, N, None) == ERR_ARG
    assert L.thx_img_scale(x, None, x, 1, 33, None) == ERR_ARG
    assert L.thx_img_scale(x, None, x, 70000, N, None) == ERR_ARG
    assert b"thx_img_scale" in L.thx_last_error()
