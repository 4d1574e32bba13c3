"""Numpy restatement of the reference's Subtract path, for test_subtract.py and
test_gpu_subtract.py, written from the reference's lines: saveSubtract
(src/Optimiser.cpp:8418-8537), the poses of saveDatabase's subtract branch
(:8295-8361), Projector::project(Image&, rot) and (rot, t) (src/Projector.cpp:
167-183, 456-464), translate on a disc and on the whole image
(src/Image/ImageFunctions.cpp:322-339, 269-284), quaternion(dvec4&, dmat33)
(src/Geometry/Euler.cpp:112-123), FFT::bwExecutePlan (src/FFT.cpp:346-360) and
centroid(const Volume&) (src/Image/ImageFunctions.cpp:37-62).

The disc is found by brute force over the half-complex grid.  The slice and the
CTF come from the C oracle (float32, as the reference holds them) through a
hand-built oracle.PixelSet; the two translation phases and everything after
them are numpy in the dtype asked for, so the same code gives the float64
reference and its own float32 error.
"""
import types

import numpy as np


def grid(N):
    """(i, j) of every stored pixel in storage order: rows j = 0 .. N/2-1,
    -N/2 .. -1, columns i = 0 .. N/2"""
    jj, i = np.mgrid[:N, :N // 2 + 1]
    return i.reshape(-1), np.where(jj < N // 2, jj, jj - N).reshape(-1)


def disc(orc, N, r, pf):
    """IMAGE_FOR_PIXEL_R_FT(r) with QUAD(i, j) < r^2 (src/Projector.cpp:170-171):
    j in [-r, r), i in [0, r], in its loop order"""
    out = []
    for j in range(-r, r):
        for i in range(0, r + 1):
            if i * i + j * j < r * r:
                out.append((i, j, (j if j >= 0 else j + N) * (N // 2 + 1) + i))
    a = np.array(out, np.int32)
    return orc.PixelSet(a[:, 0].copy(), a[:, 1].copy(), np.zeros(len(a), np.int32),
                        a[:, 2].copy(), pf)


def rot_matrix(orc, quat):
    """rotate3D (src/Geometry/Euler.cpp:181-189) as a [3, 3] matrix"""
    return orc.rotate3d(np.asarray(quat, np.float64)).reshape(3, 3).T


def quaternion(R):
    """quaternion(dvec4&, const dmat33&), src/Geometry/Euler.cpp:112-123"""
    q = np.array([0.5 * np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])),
                  0.5 * np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])),
                  0.5 * np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])),
                  0.5 * np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2]))])
    q[1] = np.copysign(q[1], R[2, 1] - R[1, 2])
    q[2] = np.copysign(q[2], R[0, 2] - R[2, 0])
    q[3] = np.copysign(q[3], R[1, 0] - R[0, 1])
    return q


def quat_matrix(q):
    """the rotation of a unit quaternion in plain numpy (to compare poses)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def phase(i, j, tx, ty, N, dtype):
    """translate(): RFLOAT rCol = nTransCol / nColRL; phase = 2 pi (i rCol +
    j rRow); COMPLEX_POLAR(-phase) -- in dtype"""
    rc, rr = dtype(tx) / dtype(N), dtype(ty) / dtype(N)
    ph = dtype(2 * np.pi) * (i.astype(dtype) * rc + j.astype(dtype) * rr)
    c = np.complex128 if dtype == np.float64 else np.complex64
    return (np.cos(-ph) + 1j * np.sin(-ph)).astype(c)


def subtract(orc, vols, vdim, pf, ori, attr, quat, trans, r, N, offS=None, dF=None, cls=None,
             symR=None, centre=None, dtype=np.float64):
    """diffFT, modelFT [1 + nSym, n, N, N/2+1], diffRL [1 + nSym, n, N, N]
    (corner origin, as FFT::bwExecutePlan leaves it), quat [1 + nSym, n, 4],
    shift [n, 2]"""
    c = np.complex128 if dtype == np.float64 else np.complex64
    n = len(ori)
    nc = N // 2 + 1
    px = disc(orc, N, r, pf)
    gi, gj = grid(N)
    symR = np.zeros((0, 3, 3)) if symR is None else np.asarray(symR, np.float64)
    copies = 1 + len(symR)
    centre = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    out = types.SimpleNamespace(
        diffFT=np.zeros((copies, n, N, nc), c), modelFT=np.zeros((copies, n, N, nc), c),
        diffRL=np.zeros((copies, n, N, N), dtype), quat=np.zeros((copies, n, 4)),
        shift=np.zeros((n, 2)))
    for l in range(n):
        t = np.asarray(trans[l], np.float64)
        off = np.zeros(2) if offS is None else np.asarray(offS[l], np.float64)
        a = np.array(attr[l], np.float32)
        if dF is not None:
            a[2] = np.float32(np.float64(a[2]) * dF[l])
            a[3] = np.float32(np.float64(a[3]) * dF[l])
        ctf = orc.ctf(px, a, N).astype(dtype)
        vol = vols[0 if cls is None else cls[l]]
        rotB = rot_matrix(orc, quat[l])
        out.shift[l] = t - off
        for s in range(copies):
            rotC = rotB if s == 0 else symR[s - 1].T @ rotB
            out.quat[s, l] = quaternion(rotC)
            # project(result, rotC, tran - offset): the slice, then translate on the disc
            P = orc.project3d(vol, vdim, pf, np.ascontiguousarray(rotC.T).reshape(-1), px)
            result = np.zeros(N * nc, c)
            result[px.iPxl] = P.astype(c) * phase(px.iCol, px.iRow, t[0] - off[0], t[1] - off[1],
                                                  N, dtype)
            model = np.zeros(N * nc, c)
            model[px.iPxl] = result[px.iPxl] * ctf
            diff = ori[l].reshape(-1).astype(c) - model
            g = rotC.T @ centre
            diff = diff * phase(gi, gj, -t[0] + off[0] - g[0], -t[1] + off[1] - g[1], N, dtype)
            out.modelFT[s, l] = model.reshape(N, nc)
            out.diffFT[s, l] = diff.reshape(N, nc)
            out.diffRL[s, l] = np.fft.irfft2(diff.reshape(N, nc), s=(N, N))
    return out


def centred(rl):
    """the corner-origin image in the centred layout of an MRC stack"""
    return np.fft.fftshift(rl, axes=(-2, -1))


def region_centroid(mask):
    """centroid(const Volume&): sum (i, j, k) u / sum u over i, j, k in
    [-N/2, N/2) of the map [k][j][i] stored with its origin at index 0"""
    N = mask.shape[0]
    c = np.zeros(3)
    w = 0.0
    for k in range(-N // 2, N // 2):
        u = np.asarray(mask[k], np.float64)               # negative k wraps, as iRL
        co = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(np.float64)
        c[0] += (u * co[None, :]).sum()
        c[1] += (u * co[:, None]).sum()
        c[2] += k * u.sum()
        w += u.sum()
    return c / w
