"""tests/recon_ref.py's float64 restatement against oracle/reconstruct.py (both
float64, numpy's FFT against torch's): equal iteration counts, the map and
the diffs within 1e-10 relative, over the options the GPU tests use."""
import numpy as np
import pytest
import torch

import recon_ref
from oracle import reconstruct as orc_rc

OPTIONS = {
    "default": {},
    "map": dict(fsc=np.linspace(0.99, 0.2, 17)),
    "map_join": dict(fsc=np.linspace(0.99, 0.2, 17), join_half=True),
    # values past both clamps on shells 5 .. 8, f = 0 past the end
    "map_edges_short": dict(fsc=np.array([0.9, 0.8, 0.7, 0.6, 0.5, 1.5, -0.2, 1.0, 0.0])),
    "no_grid_corr": dict(grid_corr=False),
    "map_no_grid_corr": dict(fsc=np.linspace(0.99, 0.2, 17), grid_corr=False),
    "max_radius": dict(max_radius=7, fsc=np.linspace(0.99, 0.2, 17)),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("N,pf", [(16, 2), (16, 3), (24, 2), (32, 1)])
def test_float64_restatement_matches_oracle(N, pf, opt):
    kw = OPTIONS[opt]
    vdim = N * pf
    T = recon_ref.sampling_density("smooth", vdim, seed=N + pf)
    if "fsc" in kw:
        # T pre-multiplied by the MAP factor, so that the balancing sees the
        # smooth T: a 1000-fold step of T between two shells (an FSC clamped
        # to 1e-3) makes the balancing amplify rounding a million times, and
        # two float64 FFT libraries then differ by more than the bound
        maxR = recon_ref.max_r(N, 1.9, kw.get("max_radius", 0))
        T = T * recon_ref.map_factor(vdim, pf, maxR, kw["fsc"], kw.get("join_half", False)).numpy()
    F = recon_ref.white_data(T, seed=7).numpy()
    ref, rit, rdiffs = orc_rc.reconstruct(F, T, N, pf, **kw)
    got, W, T_after, it, diffs = recon_ref.reconstruct(F, T, N, pf, **kw)
    assert it == rit and len(diffs) == len(rdiffs)
    assert (it > 0) == kw.get("grid_corr", True)
    if rdiffs:
        assert np.max(np.abs(np.array(diffs) - rdiffs) / np.array(rdiffs)) <= 1e-10
    assert got.dtype == torch.float64
    assert np.max(np.abs(got.numpy() - ref)) <= 1e-10 * np.max(np.abs(ref))
    # W is 0 outside the sphere, T floored
    inside = recon_ref.ft_quad(vdim) < (recon_ref.max_r(N, 1.9, kw.get("max_radius", 0)) * pf) ** 2
    assert torch.all(W[~inside] == 0) and torch.all(W[inside] > 0)
    assert float(T_after.min()) >= 1e-25


def test_float32_restatement_is_float32_and_close():
    N, pf = 16, 2
    T = recon_ref.sampling_density("smooth", N * pf, seed=3)
    F = recon_ref.white_data(T, seed=7)
    m64, W64, _, it64, _ = recon_ref.reconstruct(F, T, N, pf)
    m32, W32, T32, it32, _ = recon_ref.reconstruct(F, T, N, pf, dtype=torch.float32)
    assert m32.dtype == W32.dtype == T32.dtype == torch.float32
    assert it32 == it64
    err = float((m32.double() - m64).abs().max() / m64.abs().max())
    assert 0 < err < 1e-5


def test_hermitian_plane_average():
    vdim = 8
    T = torch.as_tensor(recon_ref.sampling_density("smooth", vdim, seed=1))
    A = recon_ref.hermitian_plane_average(T)
    assert torch.equal(A[:, :, 1:vdim // 2], T[:, :, 1:vdim // 2])
    for x in (0, vdim // 2):
        for k, j in ((0, 0), (1, 0), (3, 5), (4, 4), (7, 2)):
            want = 0.5 * (T[k, j, x] + T[(vdim - k) % vdim, (vdim - j) % vdim, x])
            assert A[k, j, x] == want
