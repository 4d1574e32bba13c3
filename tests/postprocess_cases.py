"""The inputs of the post-processing tests (tests/test_postprocess.py,
tests/test_gpu_postprocess.py), those of test_gpu_fsc_masked.py: 30 Gaussian
blobs (seed 1) plus independent white noise per half from
default_rng(int(noise 1000) + N), a soft sphere of radius 0.3 N with edge 4 as
the mask, Philox seed 11.  A case holds the float64 run of postprocess_ref, its
preconditions (asserted here, so that a failure of the inputs is not read as a
failure of the kernel), the float32 run and the bounds max(1e-5, 4 e32): absolute
for the FSC curves, relative to max|ref| for sharp and average, relative to
|bFactor| for bFactor and the Guinier ordinates.  Computed once per case and
left unchanged.  A plain module: import it from a test.
"""
import types

import numpy as np

import fsc_masked_ref
import postprocess_ref as ref

EDGE = 4.0
SEED = 11
CURVES = ("fsc", "unmasked", "masked", "randomised")
# N, pixel size, noise -> t, res, rL (the issue's table, from a float64 prototype)
CASES = {(32, 1.0, 0.02): (7, 11, 3), (32, 1.0, 0.05): (5, 9, 3), (32, 1.6, 0.05): (5, 9, 5),
         (48, 1.0, 0.05): (8, 15, 5), (48, 1.5, 0.1): (6, 13, 7)}
DEGENERATE = (32, 1.6, 0.3)     # res 6, rL 5: one fit shell

_cases = {}
_halves = {}


def blob_map(N, seed=1):
    """30 Gaussian blobs, origin at index 0, float64 (as test_gpu_fsc_masked.blob_map)"""
    rng = np.random.default_rng(seed)
    ax = np.fft.fftfreq(N, 1.0 / N)
    k, j, i = np.meshgrid(ax, ax, ax, indexing="ij")
    v = np.zeros((N, N, N))
    for c, s, a in zip(rng.uniform(-N / 5, N / 5, (30, 3)), rng.uniform(1.0, 2.5, 30),
                       rng.uniform(0.5, 1.5, 30)):
        v += a * np.exp(-((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) / (2 * s * s))
    return v


def halves(N, noise):
    """(A, B, alpha, a, b): the half-complex maps (complex64), the mask and the real halves
    (float32)"""
    key = (N, noise)
    if key not in _halves:
        v = blob_map(N)
        rng = np.random.default_rng(int(noise * 1000) + N)
        a = v + noise * v.max() * rng.standard_normal(v.shape)
        b = v + noise * v.max() * rng.standard_normal(v.shape)
        _halves[key] = (np.fft.rfftn(a).astype(np.complex64), np.fft.rfftn(b).astype(np.complex64),
                        fsc_masked_ref.soft_sphere(N, 0.3 * N, EDGE, np.float32),
                        a.astype(np.float32), b.astype(np.float32))
    return _halves[key]


def rel(x, y):
    """max |x - y| relative to max |y|"""
    return float(np.abs(np.asarray(x) - y).max() / np.abs(y).max())


def case(N, pixel_size, noise, b_factor=None, degenerate=False):
    key = (N, pixel_size, noise, b_factor)
    if key in _cases:
        return _cases[key]
    c = types.SimpleNamespace(N=N, pixel_size=pixel_size, noise=noise, b_factor=b_factor,
                              name=f"N={N} px={pixel_size} noise={noise} b={b_factor}")
    c.A, c.B, c.alpha, c.a, c.b = halves(N, noise)
    c.n_shell = N // 2 - 1
    r = c.ref = ref.postprocess(c.A, c.B, c.alpha, pixel_size, SEED, b_factor)
    t = r.thres
    # the preconditions, on the float64 reference
    assert np.all(np.abs(r.unmasked[:t + 2] - 0.8) >= 1e-3), (c.name, r.unmasked)
    assert np.all(1 - r.randomised[t + 2:] >= 0.5), (c.name, r.randomised)
    assert np.all(np.abs(r.fsc[1:r.res + 2] - 0.143) >= 1e-3), (c.name, r.fsc)
    if b_factor is None:
        assert (r.n_fit >= 2) != degenerate, (c.name, r.res, r.r_low)
    r32 = c.ref32 = ref.postprocess(c.A, c.B, c.alpha, pixel_size, SEED, b_factor, dtype=np.float32)
    assert (r32.thres, r32.res, r32.r_low) == (t, r.res, r.r_low), c.name
    c.e32 = {k: float(np.abs(getattr(r32, k) - getattr(r, k)).max()) for k in CURVES}
    c.e32["sharp"] = rel(r32.sharp, r.sharp)
    c.e32["average"] = rel(r32.average, r.average)
    if r.b_factor != 0:
        c.e32["b_factor"] = abs(r32.b_factor - r.b_factor) / abs(r.b_factor)
        c.e32["guinier"] = (float(np.abs(r32.y - r.y).max()) / abs(r.b_factor)) if len(r.y) else 0.0
    c.tol = {k: max(1e-5, 4 * e) for k, e in c.e32.items()}
    print(f"{c.name}: t = {t}, res = {r.res} of {c.n_shell}, rL = {r.r_low}, nFit = {r.n_fit}, "
          f"bFactor = {r.b_factor:.4f}, status = {r.status}; e32: "
          + ", ".join(f"{k} {e:.2e}" for k, e in c.e32.items()))
    _cases[key] = c
    return c
