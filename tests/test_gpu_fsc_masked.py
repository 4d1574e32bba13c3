"""The masked / core-region FSC on the GPU (csrc/fsc_masked.hip,
thunder_amd/resolution.py) against the float64 restatement of
tests/fsc_masked_ref.py (src/Model.cpp:411-567).

Inputs: 30 Gaussian blobs (centres within +-N/5, sigma 1 .. 2.5) plus
independent white noise of 0.02, 0.05 or 0.1 of the map's maximum per half; the
mask is a soft sphere of radius 0.3 N with edge 4, given both as alphaMask and
as coreR.  With these (checked in float64) t falls at 4 .. 11 of 15 / 23 shells
and min(1 - fscRF) over u >= t + 2 is at least 0.79.  Two conditions are asserted
on the float64 reference before anything is compared, so that a failure of the
inputs is not read as a failure of the kernel: |fscUnmask[u] - 0.8| >= 1e-3 for
u <= t + 1 (t is then the same in every precision), and min(1 - fscRF) >= 0.5
over u >= t + 2 (the unguarded divisor does not amplify).

The bound per curve is max(1e-5, 4 e32) absolute, the rule of test_gpu_noise.py
and test_gpu_subtract.py: e32 is that curve of the restatement run in float32
against its float64 run on the same inputs, computed here and printed.
"""
import types

import numpy as np
import pytest
import torch

import fsc_masked_ref as ref
from thunder_amd import mask, resolution

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CURVES = ("fsc", "unmasked", "masked", "randomised")
SHAPES = [(32, 1), (32, 2), (48, 1)]            # (N, method): 48 is hipFFT only
NOISE = [0.02, 0.05, 0.1]
EDGE = 4.0
SEED = 11


def T_(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def blob_map(N, seed=1):
    """30 Gaussian blobs, origin at index 0, float64"""
    rng = np.random.default_rng(seed)
    ax = np.fft.fftfreq(N, 1.0 / N)
    k, j, i = np.meshgrid(ax, ax, ax, indexing="ij")
    v = np.zeros((N, N, N))
    for c, s, a in zip(rng.uniform(-N / 5, N / 5, (30, 3)), rng.uniform(1.0, 2.5, 30),
                       rng.uniform(0.5, 1.5, 30)):
        v += a * np.exp(-((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) / (2 * s * s))
    return v


_cases = {}


def finish(c, seed=SEED):
    """the float64 reference, its preconditions, and the float32 error"""
    N = c.N
    c.n_shell = N // 2 - 1
    if not hasattr(c, "alpha"):
        c.radius = 0.3 * N
        c.alpha = ref.soft_sphere(N, c.radius, EDGE, np.float32)
    c.ref = ref.masked_fsc(c.A, c.B, c.n_shell, c.alpha, seed)
    t = c.ref.thres
    assert np.all(np.abs(c.ref.unmasked[:t + 2] - 0.8) >= 1e-3), (c.name, c.ref.unmasked)
    assert np.all(1 - c.ref.randomised[t + 2:] >= 0.5), (c.name, c.ref.randomised)
    r32 = ref.masked_fsc(c.A, c.B, c.n_shell, c.alpha, seed, dtype=np.float32)
    assert r32.thres == t
    c.e32 = {k: float(np.abs(getattr(r32, k) - getattr(c.ref, k)).max()) for k in CURVES}
    c.tol = {k: max(1e-5, 4 * c.e32[k]) for k in CURVES}
    print(f"{c.name}: t = {t} of {c.n_shell}, min(1 - fscRF) = "
          f"{float((1 - c.ref.randomised[t + 2:]).min()) if t + 2 < c.n_shell else 1.0:.3f}, e32 = "
          + ", ".join(f"{k} {c.e32[k]:.2e}" for k in CURVES))
    return c


def real_case(N, noise):
    key = ("real", N, noise)
    if key not in _cases:
        v = blob_map(N)
        rng = np.random.default_rng(int(noise * 1000) + N)
        c = types.SimpleNamespace(N=N, name=f"N={N} noise={noise}", map=v)
        c.A = np.fft.rfftn(v + noise * v.max() * rng.standard_normal(v.shape)).astype(np.complex64)
        c.B = np.fft.rfftn(v + noise * v.max() * rng.standard_normal(v.shape)).astype(np.complex64)
        _cases[key] = finish(c)
    return _cases[key]


def fourier_case(N):
    """independent complex noise on every stored voxel, the planes i = 0 and
    i = N/2 included: neither map is the transform of a real one"""
    key = ("fourier", N)
    if key not in _cases:
        F = np.fft.rfftn(blob_map(N))
        rng = np.random.default_rng(5 + N)
        amp = 0.05 * blob_map(N).max() * N ** 1.5 / np.sqrt(2)
        c = types.SimpleNamespace(N=N, name=f"N={N} fourier")

        def noisy():
            return (F + amp * (rng.standard_normal(F.shape) + 1j * rng.standard_normal(F.shape))
                    ).astype(np.complex64)
        c.A, c.B = noisy(), noisy()
        _cases[key] = finish(c)
    return _cases[key]


def gpu_run(c, branch="alpha", method=1, seed=SEED, A=None, B=None):
    kw = dict(mask=T_(c.alpha)) if branch == "alpha" else dict(core_radius=c.radius)
    return resolution.masked_fsc(A if A is not None else T_(c.A), B if B is not None else T_(c.B),
                                 c.n_shell, edge=EDGE, seed=seed, method=method, **kw)


def check(c, got, what):
    assert got.thres == c.ref.thres, (what, got.thres, c.ref.thres)
    for k in CURVES:
        err = float(np.abs(getattr(got, k).cpu().numpy() - getattr(c.ref, k)).max())
        print(f"{what}: {k} max |gpu - ref64| = {err:.3g} (bound {c.tol[k]:.3g})")
        assert err <= c.tol[k], (what, k, err, c.tol[k])


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("N,method", SHAPES)
def test_curves_and_threshold_match_the_reference(N, method, noise):
    c = real_case(N, noise)
    for branch in ("alpha", "core"):
        check(c, gpu_run(c, branch, method), f"{c.name} method={method} {branch}")


def test_rows_longer_than_one_wave():
    """N = 144: a row stores 73 voxels, so the shell sums take a second 64-lane chunk of every
    row, and with nShell = 71 its lanes i = 64 .. 72 feed shells 64 .. 70 (at N = 128, nShell
    63, the second chunk always starts past the last shell and contributes nothing)"""
    c = real_case(144, 0.02)
    assert c.N // 2 + 1 > 64 and c.n_shell > 64
    check(c, gpu_run(c, "alpha", 1), f"{c.name} method=1 alpha")


@pytest.mark.parametrize("N,method", SHAPES)
def test_fourier_space_noise_on_every_stored_voxel(N, method):
    c = fourier_case(N)
    for branch in ("alpha", "core"):
        check(c, gpu_run(c, branch, method), f"{c.name} method={method} {branch}")


@pytest.mark.parametrize("N,method", SHAPES)
def test_mask_and_core_branches_agree(N, method):
    c = real_case(N, 0.05)
    a, b = gpu_run(c, "alpha", method), gpu_run(c, "core", method)
    assert a.thres == b.thres
    for k in CURVES:
        err = float((getattr(a, k) - getattr(b, k)).abs().max())
        print(f"{c.name} method={method}: {k} max |alpha - core| = {err:.3g} (bound {c.tol[k]:.3g})")
        assert err <= c.tol[k], (k, err)


@pytest.mark.parametrize("N,method", SHAPES)
def test_inputs_untouched_runs_equal_seeds_differ(N, method):
    c = fourier_case(N)
    A, B = T_(c.A), T_(c.B)
    one = gpu_run(c, "alpha", method, A=A, B=B)
    assert torch.equal(A, T_(c.A)) and torch.equal(B, T_(c.B))
    two = gpu_run(c, "alpha", method, A=A, B=B)
    for k in CURVES:
        assert torch.equal(getattr(one, k), getattr(two, k)), k
    other = gpu_run(c, "alpha", method, seed=SEED + 1, A=A, B=B)
    assert not torch.equal(other.randomised, one.randomised)
    assert torch.equal(other.unmasked, one.unmasked) and torch.equal(other.masked, one.masked)
    assert other.thres == one.thres


def test_identical_halves_randomise_nothing_below_the_last_shell():
    """A = B: fscUnmask is 1 everywhere, t = nShell - 1, fsc == masked exactly"""
    c = real_case(32, 0.05)
    got = gpu_run(c, "alpha", 1, B=T_(c.A))
    assert got.thres == c.n_shell - 1
    assert float((got.unmasked - 1).abs().max()) <= 1e-12
    assert torch.equal(got.fsc, got.masked)
    assert float((got.masked - 1).abs().max()) <= 1e-6


def test_a_noise_half_gives_threshold_zero():
    N = 32
    c = types.SimpleNamespace(N=N, name="N=32 B=noise", A=real_case(N, 0.05).A)
    rng = np.random.default_rng(9)
    c.B = np.fft.rfftn(rng.standard_normal((N, N, N))).astype(np.complex64)
    finish(c)
    assert c.ref.thres == 0
    for branch in ("alpha", "core"):
        check(c, gpu_run(c, branch, 1), f"{c.name} {branch}")


def test_generated_mask_feeds_the_masked_fsc():
    """end to end: mask.gen_mask of the averaged map is the alphaMask"""
    N = 32
    base = real_case(N, 0.05)
    avg = np.fft.irfftn((base.A.astype(np.complex128) + base.B) / 2, s=(N, N, N),
                        axes=(0, 1, 2)).astype(np.float32)
    m = mask.gen_mask(T_(avg), float(np.percentile(avg, 97)), 3.0, 4.0)
    assert 0.02 < float(m.mean()) < 0.6
    c = types.SimpleNamespace(N=N, name="N=32 generated mask", A=base.A, B=base.B,
                              alpha=m.cpu().numpy())
    finish(c)
    got = resolution.masked_fsc(T_(c.A), T_(c.B), c.n_shell, mask=m, seed=SEED, method=1)
    check(c, got, c.name)
