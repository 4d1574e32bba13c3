"""numpy restatement of the masked / core-region branch of
Model::compareTwoHemispheres (src/Model.cpp:411-567) with FSC, resP and
randomPhase of src/Functions/Spectrum.cpp:302-386, written independently of
csrc/fsc_masked.hip.  The transforms are numpy.fft.irfftn / rfftn; like FFTW's
c2r they read only the Hermitian part of the planes i = 0 and i = N/2.  The
random phases are draw 0 of the package's Philox stream (q >> 32, q &
0xffffffff, tag) from tests/philox_ref.py.  ``dtype`` is the working precision
of the maps (np.float64: the reference the tests compare against; np.float32:
the same code, for the float32 error e32); shell sums are float64 either way,
as the reference's ``vec``.  A plain module: import it from a test.
"""
import types

import numpy as np

import philox_ref

TAG_A = 0x72706841           # counter word c of A's phase stream
TAG_B = 0x72706842


def shell_index(N):
    """AROUND(NORM_3(i, j, k)) over the half-complex grid [N, N, N/2+1]"""
    ax = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)
    k, j, i = np.meshgrid(ax, ax, np.arange(N // 2 + 1), indexing="ij")
    return np.rint(np.sqrt((i * i + j * j + k * k).astype(np.float64))).astype(np.int64)


def fsc(A, B, n_shell, u=None):
    """FSC(vec&, const Volume&, const Volume&)"""
    if u is None:
        u = shell_index(A.shape[0])
    m = u < n_shell

    def total(v):
        return np.bincount(u[m], weights=v[m].astype(np.float64), minlength=n_shell)
    s = total(A.real * B.real + A.imag * B.imag)
    a = total(A.real * A.real + A.imag * A.imag)
    b = total(B.real * B.real + B.imag * B.imag)
    ab = np.sqrt(a * b)
    return np.where(ab == 0, 0.0, s / np.where(ab == 0, 1.0, ab))


def res_p(f, thres, rL=1):
    """resP(fsc, thres, 1, rL, false): thres is an RFLOAT"""
    thr = float(np.float32(thres))
    r = rL
    while r < len(f) and not f[r] < thr:
        r += 1
    return r - 1


def random_phase(X, t, seed, tag, u=None):
    """randomPhase: the stored voxels of shell > t times exp(2 pi i uniform)"""
    if u is None:
        u = shell_index(X.shape[0])
    q = np.arange(X.size, dtype=np.uint64).reshape(X.shape)
    un = philox_ref.uniform(seed, q >> np.uint64(32), q & np.uint64(0xFFFFFFFF), tag, 0)
    ph = np.exp(2j * np.pi * un).astype(X.dtype)
    return np.where(u > t, X * ph, X)


def soft_sphere(N, r, ew, dtype=np.float64):
    """softMask(mask, r, ew) (src/Functions/Mask.cpp:466-487), origin at index 0"""
    ax = np.fft.fftfreq(N, 1.0 / N)
    k, j, i = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt(i * i + j * j + k * k).astype(dtype)
    r, ew = dtype(r), dtype(ew)
    edge = dtype(0.5) + dtype(0.5) * np.cos((d - r) / ew * dtype(np.pi))
    return np.where(d > r + ew, dtype(0), np.where(d >= r, edge, dtype(1))).astype(dtype)


def _masked(X, alpha, N):
    """bw, softMask with bg = 0 (v (1 - (1 - alpha))), fw"""
    rl = np.fft.irfftn(X, s=(N, N, N), axes=(0, 1, 2))
    one = alpha.dtype.type(1)
    return np.fft.rfftn(rl * (one - (one - alpha)), axes=(0, 1, 2))


def masked_fsc(A, B, n_shell, alpha, seed=0, dtype=np.float64):
    """A, B complex [N, N, N/2+1]; alpha real [N, N, N] (the caller's mask, or
    soft_sphere for the core branch).  Returns fsc, unmasked, masked,
    randomised (float64 [n_shell]) and thres."""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    A, B = np.asarray(A).astype(ctype), np.asarray(B).astype(ctype)
    alpha = np.asarray(alpha).astype(dtype)
    N = A.shape[0]
    u = shell_index(N)
    o = types.SimpleNamespace()
    o.unmasked = fsc(A, B, n_shell, u)
    o.thres = res_p(o.unmasked, 0.8)
    rA, rB = random_phase(A, o.thres, seed, TAG_A, u), random_phase(B, o.thres, seed, TAG_B, u)
    o.randomised = fsc(_masked(rA, alpha, N), _masked(rB, alpha, N), n_shell, u)
    o.masked = fsc(_masked(A, alpha, N), _masked(B, alpha, N), n_shell, u)
    idx = np.arange(n_shell)
    with np.errstate(divide="ignore", invalid="ignore"):
        o.fsc = np.where(idx < o.thres + 2, o.masked, (o.masked - o.randomised) / (1 - o.randomised))
    return o
