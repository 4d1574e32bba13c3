"""Small seeded cases of the noise-model kernels (csrc/noise.hip), one per
edge, shared by the CPU check of the reference (test_noise_edges_ref.py) and
the device check (test_gpu_noise_edges.py).  Numpy, plus synth's blob volumes.

Residual / power-spectrum / init cases (``get(name, two_d)``): two classes,
offS, dF; three images, except the grid cases, which hold one image per
on-grid rotation (eight in 3D, four in 2D).  Images are written in Fourier
space: the float32 cast of the float64 model (M for imgFT, N for oriFT) plus
independent complex noise at SNR 1 per shell on EVERY stored pixel -- column 0
below the axis included, so it is deliberately not Hermitian-consistent with
j > 0 -- and three times stronger garbage outside the disc.

  r1, r2, r3  N 8, pf 2: shell counts 1 / 1, 5 / 1, 5, 7; waves without a
              shell; at r = 1 the only pixel is the DC one
  grid-pf2    N 16, r 7 = N/2 - 1: the on-grid rotations (insert_cases.ON_GRID;
              in 2D the exact (cos, sin) of 0, 90, 180, 270 degrees): the x = 0
              column with both row signs, -0.0, the fold, weights 0 and 1,
              wrapped rows
  grid-pf1    N 16, r 6, pf 1: the largest radius pf 1 admits
  chunks3     N 96, r 46, pf 1: the shells 40, 42, 43, 44, 45 hold 133-145
              entries, a third 64-entry chunk with a partial tail
  annulus     N 32, r 12: pixels exactly on rL^2 (included) and on rNorm^2
              (excluded), rL = 0, rNorm = r - 1/2, rL = rNorm, a fractional
              pair whose squares are no float32
  weak        N 16, r 7: img = the float32 model itself, residual << signal

3D rotations are uniform quaternions redrawn until ``fused_agree3`` holds; 2D
ones come from twod_cases.draw_rot (fold and floor decided alike in FP32 and
FP64, fused or not); the on-grid ones are kept as given and checked.
"""
import types

import numpy as np

import insert_cases
import noise_edges_ref as R
import twod_cases as T2C
from thunder_amd import synth

SPEC = {   # name: (N, r, pf, radii pairs)
    "r1": (8, 1, 2, [(0.0, 0.5)]),
    "r2": (8, 2, 2, [(0.0, 1.5), (1.0, 1.5)]),
    "r3": (8, 3, 2, [(0.0, 2.5), (1.0, 2.0)]),
    "grid-pf2": (16, 7, 2, [(1.0, 6.5)]),
    "grid-pf1": (16, 6, 1, [(1.0, 5.5)]),
    "chunks3": (96, 46, 1, [(2.0, 45.5)]),
    "annulus": (32, 12, 2, [(5.0, 10.0), (0.0, 11.5), (7.0, 7.0), (2.3, 9.7), (0.0, 5.0)]),
    "weak": (16, 7, 2, [(1.0, 6.5)]),
}
NAMES = list(SPEC)
ON_RL2 = [(3, 4), (4, 3), (5, 0), (0, 5), (0, -5), (3, -4), (4, -3)]         # on 5^2: included
ON_RN2 = [(6, 8), (8, 6), (10, 0), (0, 10), (0, -10), (6, -8), (8, -6)]      # on 10^2: excluded

_vols, _cache = {}, {}


def volumes(N, pf, two_d):
    key = (N, pf, two_d)
    if key not in _vols:
        if two_d:
            _vols[key] = T2C.classes(2, N, pf, 40 + N + pf)
        else:
            _vols[key] = np.stack([synth.projectee(synth.blob_volume(N, n_blobs=30, seed=s), pf).numpy()
                                   for s in (1, 2)])
    return _vols[key]


def _draw3(rng, n, px, pf):
    q = synth.uniform_quaternions(n, rng)
    for _ in range(100):
        bad = np.flatnonzero(~R.fused_agree3(R.mats3(q), px.iCol, px.iRow, pf))
        if not len(bad):
            return q
        q[bad] = synth.uniform_quaternions(len(bad), rng)
    raise AssertionError("no clean rotation found")


def _noise(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def get(name, two_d):
    key = (name, two_d)
    if key in _cache:
        return _cache[key]
    N, r, pf, radii = SPEC[name]
    seed = 7000 + 10 * NAMES.index(name) + int(two_d)
    rng = np.random.default_rng(seed)
    px = R.pixels(N, r)
    if name.startswith("grid"):
        rot = T2C.GRID.copy() if two_d else insert_cases.ON_GRID.copy()
    elif two_d:
        rot = T2C.draw_rot(rng, 3, px.iCol, px.iRow, pf)
    else:
        rot = _draw3(rng, 3, px, pf)
    n = len(rot)
    c = types.SimpleNamespace(
        name=name, two_d=two_d, N=N, r=r, pf=pf, vdim=N * pf, radii=radii, px=px,
        vols=volumes(N, pf, two_d), rot=np.ascontiguousarray(rot, np.float64),
        attr=synth.ctf_attrs(n, seed=seed + 5), trans=rng.standard_normal((n, 2)) * 2,
        off=rng.standard_normal((n, 2)) * 1.5, dF=1.0 + 0.02 * rng.standard_normal(n),
        cls=(np.arange(n) % 2)[::-1].astype(np.int32).copy())
    shape = (n, N, N // 2 + 1)
    c.img, c.ori = np.zeros(shape, np.complex64), np.zeros(shape, np.complex64)
    in_disc = np.zeros(N * (N // 2 + 1), bool)
    in_disc[px.iPxl] = True
    for l in range(n):
        M, _, Nn, _ = R.models(c, l, px, 1)
        for dst, sig in ((c.img, M), (c.ori, Nn)):
            full = np.zeros(N * (N // 2 + 1), np.complex128)
            amp = np.sqrt(np.maximum(R.shell_mean(R.p2(sig), px), 1e-6) / 2)[px.iSig]
            if name != "weak":
                full[~in_disc] = 3 * amp.max() * _noise(rng, np.count_nonzero(~in_disc))
                full[px.iPxl] = amp * _noise(rng, px.n)
            full[px.iPxl] += sig
            dst[l] = full.reshape(N, N // 2 + 1).astype(np.complex64)
    _cache[key] = c
    return c


def ref(c, margin):
    """noise_edges_ref.residual of the case, computed once per margin"""
    key = ("ref", c.name, c.two_d, margin)
    if key not in _cache:
        _cache[key] = R.residual(c, margin)
    return _cache[key]


# ----------------------------------------------------------------- accumulate
ACC_N = (1, 7, 8, 9, 16, 17, 65)
ACC_SHAPE = ((1, 1), (3, 10), (3, 31), (5, 63))     # (3, 31): 96 elements, a partial second block
ACC_SPLIT = ((8, 9), (5, 12))                       # at a batch boundary and off it


def acc_case(n, n_group, r):
    """Positive float32 spectra [n, 4, r]; the last image alone in the last
    group with values 1e3 times the others, group 1 (of three or more) empty;
    ``nan``: the same with one image's shell of zero power (rows 2 and 3 zero:
    0 / 0) and, where there is room, another with |img|^2 = 0 alone (x / 0)."""
    rng = np.random.default_rng(8000 + 100 * n + 10 * n_group + r)
    s = (10.0 ** rng.uniform(-2, 1, (n, 4, r))).astype(np.float32)
    s[-1] *= np.float32(1e3)
    if n_group == 1:
        group = np.zeros(n, np.int32)
    else:
        pool = np.array([g for g in range(n_group - 1) if g != 1], np.int32)
        group = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        group[-1] = n_group - 1
    bad = s.copy()
    l, u = (n - 1) // 2, r // 2
    bad[l, 2:, u] = 0
    if n > 2 and r > 1:
        bad[0, 3, r - 1] = 0
    return types.SimpleNamespace(spectra=s, group=group, nan=bad, at=(l, u), n_group=n_group, r=r)


# ------------------------------------------------------------------------ rows
ROWS_N = (8192, 8193, 20000)                        # 20000 takes three trips


def rows_case(n_pxl):
    """sigRcp [3, 9] float64 no float32 holds exactly; iSig with -1, nCol - 1
    and nCol in it, at the ends and across the trips' seams; groups with -1 and
    nGroup."""
    rng = np.random.default_rng(8500 + n_pxl)
    n_group, n_col = 3, 9
    rcp = -0.5 / 10.0 ** rng.uniform(-3, 3, (n_group, n_col))
    i_sig = rng.integers(0, n_col, n_pxl).astype(np.int32)
    for at, v in ((0, -1), (1, n_col - 1), (2, n_col), (8191, n_col - 1), (n_pxl - 1, n_col - 1),
                  (n_pxl - 2, -1), (n_pxl - 3, n_col)):
        i_sig[at] = v
    group = np.array([2, -1, 0, n_group, 1], np.int32)
    return types.SimpleNamespace(rcp=rcp, iSig=i_sig, group=group, n_group=n_group, n_col=n_col,
                                 px=types.SimpleNamespace(iSig=i_sig, n=n_pxl))


# ----------------------------------------------------------------------- scale
SCALE_N = (180, 182)                                # per 16380: 64 blocks, one trip; 16744: a second trip
SCALE = np.array([0.0, -1.0, 1.0], np.float32), np.array([0.37, -2.5, 1e-3], np.float32)


def scale_case(N):
    rng = np.random.default_rng(8700 + N)
    shape = (5, N, N // 2 + 1)
    mk = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return types.SimpleNamespace(img=mk(), ori=mk())
