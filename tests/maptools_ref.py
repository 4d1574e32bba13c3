"""Float64 numpy restatement of the map tools (csrc/maptools.hip), written from
the reference and independently of the kernels:

  transform   VOL_TRANSFORM_MAT_RL / SYMMETRIZE_RL (include/Geometry/Transformation.h:58-84,
              139-163) with Volume::getByInterpolationRL (src/Image/Volume.cpp:296-312, 482-489)
  ft_resize   thunder_resize's copy (appsrc/thunder_resize.cpp:149-163)
  resize      fw, ft_resize, bw (1 / M^3)
  project     Projector::project(Image&, mat) (src/Projector.cpp:276-294) with
              Volume::getByInterpolationFT (src/Image/Volume.cpp:314-338), translate's phase
              (src/Image/ImageFunctions.cpp:233-252) and FFT::bw (1 / N^2)
  soft_mask   softMask(dst, src, r, ew, 0) (src/Functions/Mask.cpp:499-521)
  align_z     alignZ (src/Geometry/Euler.cpp:239-270)

Maps are real [N, N, N] with the origin at [0, 0, 0] and negatives wrapped, indexed [k][j][i];
transforms are half-complex [N, N, N/2+1], unnormalised.  ``dtype`` is the precision of the
coordinates handed to the interpolation, of the taps, the weights and the sums
(np.float32: the reference's RFLOAT); the matrix product and the ball test are float64 either
way, as in the reference.
"""
import numpy as np


def signed(N):
    """the signed coordinate of every wrapped index: 0 .. N/2-1, -N/2 .. -1"""
    return np.fft.fftfreq(N, 1.0 / N).astype(np.int64)


def grid3(N):
    ax = signed(N)
    return np.meshgrid(ax, ax, ax, indexing="ij")       # k, j, i


def rotated(M, i, j, k):
    """M (i, j, k) and its squared norm in float64, left to right"""
    M = np.asarray(M, np.float64).reshape(3, 3)
    x = M[0, 0] * i + M[0, 1] * j + M[0, 2] * k
    y = M[1, 0] * i + M[1, 1] * j + M[1, 2] * k
    z = M[2, 0] * i + M[2, 1] * j + M[2, 2] * k
    return x, y, z, x * x + y * y + z * z


def interp_rl(src, x, y, z, dtype):
    """floor-based trilinear, taps added in box order k, j, i; wrapped indices"""
    N = src.shape[0]
    x, y, z = (np.asarray(v).astype(dtype) for v in (x, y, z))
    f = [np.floor(v) for v in (x, y, z)]
    d = [v - fv for v, fv in zip((x, y, z), f)]
    x0, y0, z0 = (fv.astype(np.int64) for fv in f)
    one = dtype(1)
    w = [(one - dv, dv) for dv in d]
    acc = np.zeros(x.shape, dtype)
    s = src.astype(dtype)
    for c in range(2):
        for b in range(2):
            for a in range(2):
                tap = s[(z0 + c) % N, (y0 + b) % N, (x0 + a) % N]
                acc = (acc + (tap * ((w[0][a] * w[1][b]).astype(dtype) * w[2][c]).astype(dtype)
                              ).astype(dtype)).astype(dtype)
    return acc


def nearest_rl(src, x, y, z, dtype):
    N = src.shape[0]
    xi, yi, zi = (np.rint(np.asarray(v).astype(dtype)).astype(np.int64) for v in (x, y, z))
    return src.astype(dtype)[zi % N, yi % N, xi % N]


def lattice_ties(N, r):
    """the voxels with i^2 + j^2 + k^2 == r^2 exactly (none unless r^2 is an integer): under a
    generic rotation their |M x|^2 rounds to either side of the strict compare"""
    k, j, i = grid3(N)
    return (i * i + j * j + k * k).astype(np.float64) == float(r) * float(r)


def transform(src, mats, r, interp="linear", add_src=False, dtype=np.float64, ties=None):
    """out(x) = (add_src ? src(x) : 0) + sum_m [|M_m x|^2 < r^2] interp(src, M_m x), the
    matrices in index order.  ties "in" / "out" puts the lattice_ties voxels inside / outside
    the ball whatever the rounding of |M x|^2 says (None: the compare as computed)."""
    N = src.shape[0]
    k, j, i = grid3(N)
    acc = src.astype(dtype).copy() if add_src else np.zeros((N, N, N), dtype)
    fn = interp_rl if interp == "linear" else nearest_rl
    tie = lattice_ties(N, r)
    for M in np.asarray(mats, np.float64).reshape(-1, 3, 3):
        x, y, z, q2 = rotated(M, i, j, k)
        inside = q2 < float(r) * float(r)
        if ties is not None:
            inside = (inside | tie) if ties == "in" else (inside & ~tie)
        v = np.zeros((N, N, N), dtype)
        v[inside] = fn(src, x[inside], y[inside], z[inside], dtype)
        acc = (acc + v).astype(dtype)
    return acc


def permuted(v, M):
    """v(M x) for a signed permutation M, by index arithmetic alone"""
    N = v.shape[0]
    k, j, i = grid3(N)
    M = np.asarray(M).astype(np.int64)
    x, y, z = (M[a, 0] * i + M[a, 1] * j + M[a, 2] * k for a in range(3))
    return v[z % N, y % N, x % N]


def ball(N, r):
    k, j, i = grid3(N)
    return (i * i + j * j + k * k).astype(np.float64) < float(r) * float(r)


def ft_resize(ft, M):
    N = ft.shape[0]
    L = min(N, M)
    out = np.zeros((M, M, M // 2 + 1), ft.dtype)
    jk = np.arange(-L // 2, L // 2)
    out[np.ix_(jk % M, jk % M, np.arange(L // 2 + 1))] = ft[np.ix_(jk % N, jk % N,
                                                                 np.arange(L // 2 + 1))]
    return out


def resize(vol, M, dtype=np.float64):
    """thunder_resize: irfftn reads the Hermitian part of planes i = 0 and i = M/2, as FFTW's
    c2r, and carries the 1 / M^3; nothing is renormalised"""
    ft = np.fft.rfftn(np.asarray(vol).astype(dtype))
    return np.fft.irfftn(ft_resize(ft, M), s=(M, M, M), axes=(0, 1, 2)).astype(dtype)


def quat_to_mat(q):
    """rotate3D (src/Geometry/Euler.cpp:181-189): R = I + 2 q0 A + 2 A A"""
    q = np.asarray(q, np.float64)
    A = np.array([[0, -q[3], q[2]], [q[3], 0, -q[1]], [-q[2], q[1], 0]])
    return np.eye(3) + 2 * q[0] * A + 2 * A @ A


def interp_ft(vol, x, y, z, dtype):
    """Hermitian fold for x < 0, floor + 8 weights, taps in box order k, j, i"""
    vdim = vol.shape[0]
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    x, y, z = (np.asarray(v).astype(dtype) for v in (x, y, z))
    conj = ~(x >= 0)
    x, y, z = (np.where(conj, -v, v) for v in (x, y, z))
    f = [np.floor(v) for v in (x, y, z)]
    d = [(v - fv).astype(dtype) for v, fv in zip((x, y, z), f)]
    x0, y0, z0 = (fv.astype(np.int64) for fv in f)
    one = dtype(1)
    w = [(one - dv, dv) for dv in d]
    acc = np.zeros(x.shape, ctype)
    s = vol.astype(ctype)
    for c in range(2):
        for b in range(2):
            for a in range(2):
                wt = ((w[0][a] * w[1][b]).astype(dtype) * w[2][c]).astype(dtype)
                acc = (acc + (s[(z0 + c) % vdim, (y0 + b) % vdim, x0 + a] * wt).astype(ctype)
                       ).astype(ctype)
    return np.where(conj, np.conj(acc), acc)


def hermitian_cols(img):
    """columns i = 0 and i = N/2 of half-complex images [..., N, N/2+1] <- their Hermitian part"""
    out = img.copy()
    N = img.shape[-2]
    neg = (-np.arange(N)) % N
    for col in (0, N // 2):
        v = img[..., :, col]
        out[..., :, col] = (v + np.conj(v[..., neg])) / 2
    return out


def project(vol, mats, N, pf=2, r=None, trans=None, dtype=np.float64):
    """(imgFT [n, N, N/2+1], imgRL [n, N, N]); mats [n, 3, 3] (x' = M x)"""
    r = N // 2 - 1 if r is None else r
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    mats = np.asarray(mats, np.float64).reshape(-1, 3, 3)
    j, i = np.meshgrid(signed(N), np.arange(N // 2 + 1), indexing="ij")
    disc = i * i + j * j < r * r
    out = np.zeros((len(mats), N, N // 2 + 1), ctype)
    for m, M in enumerate(mats):
        nx, ny = (pf * i[disc]).astype(np.float64), (pf * j[disc]).astype(np.float64)
        x, y, z = (M[a, 0] * nx + M[a, 1] * ny for a in range(3))
        v = interp_ft(vol, x, y, z, dtype)
        if trans is not None:
            tx, ty = (dtype(t) / dtype(N) for t in trans[m])
            rev = -(i[disc].astype(dtype) * tx + j[disc].astype(dtype) * ty).astype(dtype)
            v = (v * np.exp(2j * np.pi * rev.astype(np.float64)).astype(ctype)).astype(ctype)
        out[m][disc] = v
    rl = np.fft.irfft2(hermitian_cols(out), s=(N, N)).astype(dtype)
    return out, rl


def soft_mask(vol, r, ew, dtype=np.float64):
    N = vol.shape[0]
    k, j, i = grid3(N)
    u = np.sqrt((i * i + j * j + k * k).astype(dtype))
    r, ew, half = dtype(r), dtype(ew), dtype(0.5)
    with np.errstate(invalid="ignore"):
        w = (half - half * np.cos((u - r) / ew * dtype(np.pi))).astype(dtype)   # the background's share
    keep = np.where(u > r + ew, dtype(0), np.where(u >= r, dtype(1) - w, dtype(1))).astype(dtype)
    return (np.asarray(vol).astype(dtype) * keep).astype(dtype)


def align_z(v):
    x, y, z = (float(c) for c in v)
    p_yz, p = np.sqrt(y * y + z * z), np.sqrt(x * x + y * y + z * z)
    if p_yz / p > 1e-2:
        return np.array([[p_yz, -x * y / p_yz, -x * z / p_yz], [0, z / p_yz, -y / p_yz],
                         [x / p, y / p, z / p]])
    return np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])
