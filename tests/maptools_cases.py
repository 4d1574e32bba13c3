"""The inputs and bounds of the map-tool tests (tests/test_gpu_maptools.py).  A volume is the
package's blob volume (synth.blob_volume, seed 1) moved to the origin-at-index-0 layout plus 2 %
white noise from default_rng(N), so that no tap is zero.  A case holds the float64 run of
maptools_ref, its float32 run and, per compared array, e32 = max|ref32 - ref64| / max|ref64| and
the bound max(1e-5, 4 e32): the reference's own float32 error sets the bound, never the code
under test (tests/postprocess_cases.py's rule).  Computed once per case and left unchanged.
A plain module: import it from a test.
"""
import types

import numpy as np
import torch

import maptools_ref as ref
from thunder_amd import synth

_vols = {}
_cases = {}

RNG_MAT = 7         # the seed of the generic rotations


def volume(N):
    """float32 [N, N, N], origin at index 0"""
    if N not in _vols:
        v = np.fft.ifftshift(synth.blob_volume(N).numpy().astype(np.float64))
        v = v + 0.02 * v.max() * np.random.default_rng(N).standard_normal(v.shape)
        _vols[N] = v.astype(np.float32)
    return _vols[N]


def projectee(N, pf=2):
    """complex64 [pf N, pf N, pf N/2+1]: the padded transform of volume(N) (synth.projectee)"""
    key = ("proj", N, pf)
    if key not in _vols:
        centred = torch.as_tensor(np.fft.fftshift(volume(N)))
        _vols[key] = synth.projectee(centred, pf).numpy()
    return _vols[key]


def generic_quats(n, seed=RNG_MAT):
    q = np.random.default_rng(seed).standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def generic_mats(n, seed=RNG_MAT):
    return np.stack([ref.quat_to_mat(q) for q in generic_quats(n, seed)])


def axis_turns():
    """90 degrees about x, y and z: exact signed permutations"""
    return np.array([[[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                     [[0, -1, 0], [1, 0, 0], [0, 0, 1]]], np.float64)


def c4_elements():
    """the non-identity elements of C4 about z, exact"""
    t = axis_turns()[2]
    return np.stack([t, t @ t, t @ t @ t])


def rel(x, y):
    """max |x - y| relative to max |y|"""
    return float(np.abs(np.asarray(x) - y).max() / np.abs(y).max())


def _bounded(name, run):
    """run(dtype) -> dict of arrays; the case with ref, ref32, e32 and tol per array"""
    if name not in _cases:
        c = types.SimpleNamespace(name=name, ref=run(np.float64), ref32=run(np.float32))
        c.e32 = {k: rel(c.ref32[k], c.ref[k]) for k in c.ref}
        c.tol = {k: max(1e-5, 4 * e) for k, e in c.e32.items()}
        print(f"{name}: e32 " + ", ".join(f"{k} {e:.2e}" for k, e in c.e32.items()))
        _cases[name] = c
    return _cases[name]


def transform_case(N, mats, r, interp="linear", add_src=False, tag="", ties=None):
    """ties "in" / "out": the lattice points at exactly |x| = r forced to one side of the ball
    test (maptools_ref.transform)"""
    mats = np.asarray(mats, np.float64).reshape(-1, 3, 3)
    return _bounded(f"transform N={N} r={r} {interp} add={add_src} n={len(mats)} ties={ties} {tag}",
                    lambda dt: {"out": ref.transform(volume(N), mats, r, interp, add_src, dt, ties)})


def resize_case(N, M):
    return _bounded(f"resize {N}->{M}", lambda dt: {"out": ref.resize(volume(N), M, dt)})


def project_case(N, n, r, with_trans, pf=2):
    mats = generic_mats(n, RNG_MAT + n)
    trans = np.random.default_rng(n).uniform(-3, 3, (n, 2)) if with_trans else None

    def run(dt):
        ft, rl = ref.project(projectee(N, pf), mats, N, pf, r, trans, dt)
        return {"ft": ft, "rl": rl}
    c = _bounded(f"project N={N} n={n} r={r} trans={with_trans}", run)
    c.mats, c.trans = mats, trans
    return c


def soft_mask_case(N, r, ew):
    return _bounded(f"soft_mask N={N} r={r} ew={ew}",
                    lambda dt: {"out": ref.soft_mask(volume(N), r, ew, dt)})


def check(c, key, got, excused=None):
    """print the bound, the error and e32, then assert; excused: a mask of elements left out"""
    want = c.ref[key]
    diff = np.abs(np.asarray(got) - want)
    if excused is not None:
        diff = np.where(excused, 0.0, diff)
    err = float(diff.max() / np.abs(want).max())
    print(f"{c.name} [{key}]: bound {c.tol[key]:.2e}, error {err:.2e}, e32 {c.e32[key]:.2e}")
    assert np.all(np.isfinite(np.asarray(got).view(np.float32))), c.name
    assert err <= c.tol[key], (c.name, key, err, c.tol[key])
    return err
