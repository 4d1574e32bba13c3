"""Float64 numpy restatement of the reference's noise model, for test_noise.py
and test_gpu_noise.py: powerSpectrum (src/Functions/Spectrum.cpp:161-190),
Optimiser::allReduceSigma (src/Optimiser.cpp:6395-6709), normCorrection
(:6201-6393) and initSigma (:5145-5243) under the reference's active switches.

The pixel domain is found by brute force over the half-complex grid, never
from thx_spectrum_pixels.  The slice, the CTF and the translation phase come
from the C oracle through a hand-built oracle.PixelSet that covers the full
disc (column 0 with j < 0 included); everything after them is numpy in the
dtype asked for, so the same code gives the float64 reference and its own
float32 error.
"""
import numpy as np


def domain(N, r):
    """powerSpectrum's pixels in its loop order (j outer, i inner): (iCol,
    iRow, iShell, iPxl) over j in [-N/2, N/2), i in [0, N/2]."""
    out = []
    for j in range(-N // 2, N // 2):
        for i in range(0, N // 2 + 1):
            if i * i + j * j < r * r:
                u = int(np.rint(np.hypot(i, j)))
                if u < r:
                    out.append((i, j, u, (j if j >= 0 else j + N) * (N // 2 + 1) + i))
    a = np.array(out, np.int32)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()


def by_shell(N, r):
    """the same pixels listed shell by shell, loop order kept inside a shell,
    plus shellStart [r + 1]"""
    iCol, iRow, iShell, iPxl = domain(N, r)
    o = np.argsort(iShell, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(iShell, minlength=r))]).astype(np.int32)
    return iCol[o], iRow[o], iShell[o], iPxl[o], start


def disc(orc, N, r, pf):
    iCol, iRow, iShell, iPxl = domain(N, r)
    return orc.PixelSet(iCol, iRow, iShell, iPxl, pf)


def shell_means(v, iShell, r, dtype=np.float64):
    """mean of v per shell, summed in dtype"""
    v = np.asarray(v, dtype)
    return np.array([v[iShell == u].sum(dtype=dtype) / dtype(np.count_nonzero(iShell == u))
                     for u in range(r)], dtype)


def power_spectrum(img, px, r, dtype=np.float64):
    c = np.complex128 if dtype == np.float64 else np.complex64
    v = img.reshape(-1)[px.iPxl].astype(c)
    return shell_means(v.real * v.real + v.imag * v.imag, px.iSig, r, dtype)


def rot2(th):
    return np.array([np.cos(th), np.sin(th)], np.float64)


def slice_terms(orc, px, vol, vdim, pf, rot, attr, d, N):
    """(P, ctf) on the disc: the class's Fourier slice at rot (a quaternion, or
    2D (cos, sin)) and the CTF at (dU d, dV d), float32 as the reference
    holds them"""
    if len(rot) == 2:
        P = orc.project2d(vol, vdim, pf, rot, px)
    else:
        P = orc.project3d(vol, vdim, pf, orc.rotate3d(rot), px)
    a = np.array(attr, np.float32)
    if d is not None:
        a[2] = np.float32(np.float64(a[2]) * d)
        a[3] = np.float32(np.float64(a[3]) * d)
    return P, orc.ctf(px, a, N)


def model(orc, px, P, ctf, t, N, dtype=np.float64):
    """CTF P(t) on the disc in dtype"""
    c = np.complex128 if dtype == np.float64 else np.complex64
    ph = orc.translate(px, float(t[0]), float(t[1]), N)
    return ctf.astype(dtype) * (P.astype(c) * ph.astype(c))


def residual_spectra(orc, px, r, vols, vdim, pf, img, ori, attr, rot, trans, off, dF, cls, N,
                     norm_radii=None, dtype=np.float64):
    """[n, 4, r] shell means of |img - M|^2, |ori - N|^2, |M|^2, |img|^2 and
    norm [n] (pixels with rL^2 <= i^2+j^2 < rNorm^2)"""
    c = np.complex128 if dtype == np.float64 else np.complex64
    n = len(img)
    out = np.zeros((n, 4, r), dtype)
    norm = np.zeros(n, dtype)
    quad = px.iCol.astype(np.int64) ** 2 + px.iRow.astype(np.int64) ** 2
    for l in range(n):
        P, ctf = slice_terms(orc, px, vols[cls[l]], vdim, pf, rot[l], attr[l],
                             None if dF is None else dF[l], N)
        M = model(orc, px, P, ctf, trans[l], N, dtype)
        Nn = model(orc, px, P, ctf, trans[l] - off[l], N, dtype)
        a = img[l].reshape(-1)[px.iPxl].astype(c)
        b = ori[l].reshape(-1)[px.iPxl].astype(c)

        def p2(z):
            return z.real * z.real + z.imag * z.imag
        res = p2(a - M)
        for q, v in enumerate((res, p2(b - Nn), p2(M), p2(a))):
            out[l, q] = shell_means(v, px.iSig, r, dtype)
        if norm_radii is not None:
            rL, rN = norm_radii
            norm[l] = res[(quad >= rL * rL) & (quad < rN * rN)].sum(dtype=dtype)
    return out, norm


def sigma_sums(spectra, group, n_group):
    """acc [3][nGroup][r+1] of allReduceSigma's loop (group 0-based; None = row 0)"""
    n, _, r = spectra.shape
    s = spectra.astype(np.float64)
    acc = np.zeros((3, n_group, r + 1))
    for l in range(n):
        g = 0 if group is None else group[l]
        acc[0, g, :r] += s[l, 0] / 2
        acc[1, g, :r] += s[l, 1] / 2
        acc[2, g, :r] += np.sqrt(s[l, 2] / s[l, 3])
        acc[:, g, r] += 1
    return acc


def sigma_finalise(acc, n_col, alpha, grouped):
    _, n_group, r1 = acc.shape
    r = r1 - 1
    m = np.zeros((3, n_group, n_col - 1))
    for g in range(n_group):
        src = g if grouped else 0
        m[:, g, :r] = acc[:, src, :r] / acc[:, src, r:r + 1]
    m[:, :, r:] = m[:, :, r - 1:r]
    ratio = np.minimum(1.0, m[2])
    sig = np.zeros((n_group, n_col))
    rcp = np.zeros((n_group, n_col))
    sig[:, :-1] = ratio * m[0] + (1 - ratio) * alpha * m[1]
    rcp[:, :-1] = -0.5 / sig[:, :-1]
    return sig, rcp


def init_sums(ori, px, r):
    """(avgSum [N][N/2+1] complex128, psSum [r]) of initSigma"""
    avg = np.sum(np.asarray(ori, np.complex128), axis=0)
    ps = np.zeros(r)
    for o in ori:
        ps += power_spectrum(o, px, r)
    return avg, ps


def init_finalise(avg_sum, ps_sum, n_total, px, r, n_group, n_col):
    avg = avg_sum.reshape(-1)[px.iPxl] / n_total
    ps_avg = shell_means(avg.real + avg.imag, px.iSig, r) ** 2
    s = np.zeros(n_col - 1)
    s[:r] = (ps_sum / n_total - ps_avg) / 2
    s[r:] = s[r - 1]
    sig = np.zeros((n_group, n_col))
    rcp = np.zeros((n_group, n_col))
    sig[:, :-1] = s
    rcp[:, :-1] = -0.5 / s
    return sig, rcp
