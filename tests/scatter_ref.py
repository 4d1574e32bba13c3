"""Float64 reference of the weighted trilinear back-projection and gather,
with a per-voxel rounding budget (test infrastructure, host only).

``insert_f64`` restates Reconstructor::insertP / Volume::addFT
(src/Reconstructor.cpp:782-863, src/Image/Volume.cpp:340-375) as the oracle's
``orc_insert_batch`` does: the rotation matrix comes from ``orc.rotate3d``, the
rotated coordinate is formed in FP64 and rounded to FP32 exactly as there, so
the reference, the oracle and the kernels take the same fold and floor
decisions.  Everything after that is float64: the fractions ``x - floor(x)``
(exact), the phase ``exp(+2 pi i (iCol dx + iRow dy) / N)`` with
``(dx, dy) = trans - off``, ``val = dat phase ctf w``, ``tv = ctf^2 w``, the
conjugation when ``!(x >= 0)``, the 8 taps with rows and slices wrapped, and
the sum (``np.add.at``).

The budget of voxel v, with u = 2^-24, over the taps that reach v:

    b_v = u [ sum |val| (3 + wt (10 + 4 P theta)) + n_v sum |val| wt ]

  3        each of the three weight factors carries an absolute error <= u
           from ``c - floor(c)`` and ``1 - xd`` in FP32, so wt is off by <= 3 u
  10       the relative roundings of the complex product, the CTF and w
           products and the weight product
  4 theta  the FP32 phase has about four roundings of magnitude
           theta = 2 pi (|iCol dx| + |iRow dy|) / N (the absolute-sum form: the
           two terms round separately, and |sum| under-bounds when they cancel)
  n_v ...  FP32 summation of the n_v taps in any order
  P        the phase margin: 1 for the oracle (libm sin / cos), 4 for the
           device, the project's rule for every phase_shift output
           (max(1e-5, 4 e32) in test_gpu_round.py: the hardware sin / cos of
           revolutions are a factor ~4 behind the FP32 phase's own rounding)

T uses the same form with tv in place of |val| and no phase term.  The binned
deposit rounds every tap product once on a fixed-point grid of 2^-48 of the
batch's largest entry of its kind (insert_binned.hip), i.e. by at most
2^-47 vmax: ``binned=True`` adds n_v 2^-47 vmax.  Nothing else is in the
budget; in particular there is no floor relative to max |F|.

The CTF-search variant (``attr`` / ``nD``) evaluates the CTF in float64 from
the formula of common.h:ctf_at; the FP32 formula's own error is absolute in
the CTF, not relative (its argument ki reaches hundreds of radians), so that
variant adds |dat| w dctf wt per tap to F and (2 |ctf| + dctf) dctf w wt to T,
with dctf bounded from ctf_at's roundings (see ``ctf_f64``).
"""
import numpy as np

U32 = 2.0 ** -24


def _mats(quat):
    from oracle import oracle
    q = np.ascontiguousarray(quat, np.float64).reshape(-1, 4)
    return np.stack([oracle.rotate3d(x) for x in q])         # [S, 9] column-major


def coords_f32(mat, iCol, iRow, pf):
    """R (iCol pf, iRow pf, 0) in FP64, rounded to FP32: [S, nPxl] x, y, z."""
    X = (np.asarray(iCol, np.int64) * pf).astype(np.float64)[None, :]
    Y = (np.asarray(iRow, np.int64) * pf).astype(np.float64)[None, :]
    m = mat[:, :, None]
    return ((m[:, 0] * X + m[:, 3] * Y).astype(np.float32),
            (m[:, 1] * X + m[:, 4] * Y).astype(np.float32),
            (m[:, 2] * X + m[:, 5] * Y).astype(np.float32))


def fold_taps(x, y, z, vdim):
    """conjHalf + WG_TRI_INTERP_LINEAR on FP32 coordinates: (conj, idx [8, ...],
    wt [8, ...] float64, corner (x0, y0, z0) int64); taps in box order k, j, i."""
    conj = ~(x >= 0)
    sgn = np.where(conj, np.float32(-1), np.float32(1))
    c = [x * sgn, y * sgn, z * sgn]
    c0 = [np.floor(a) for a in c]
    fr = [a.astype(np.float64) - b.astype(np.float64) for a, b in zip(c, c0)]   # exact
    i0 = [b.astype(np.int64) for b in c0]
    ncol = vdim // 2 + 1
    assert i0[0].min() >= 0 and i0[0].max() + 1 < ncol, "tap outside the half-complex row"
    assert max(np.abs(i0[1]).max(), np.abs(i0[2]).max()) + 1 < vdim, "row / slice outside the box"
    idx, wt = [], []
    for k in range(2):
        for j in range(2):
            for i in range(2):
                zz, yy = i0[2] + k, i0[1] + j
                zz = np.where(zz >= 0, zz, zz + vdim)
                yy = np.where(yy >= 0, yy, yy + vdim)
                idx.append((zz * vdim + yy) * ncol + i0[0] + i)
                wt.append((fr[0] if i else 1 - fr[0]) * (fr[1] if j else 1 - fr[1]) *
                          (fr[2] if k else 1 - fr[2]))
    return conj, np.stack(idx), np.stack(wt), i0


def ctf_f64(attr, d, iCol, iRow, N):
    """common.h:ctf_at (src/CTF.cpp:113-151) in float64 for attr [8] at the
    defocus factors d [M]: (ctf [M, nPxl], dctf [M, nPxl]).

    dctf bounds the FP32 formula's absolute error.  With ki = t1 + t2 - ps,
    t1 = K1 defocus u^2 and t2 = K2 u^4, counting relative roundings:
      t1: K1 2 (lambda, pi lambda); defocus 4 (dU d and dV d, sum, product,
          sum); u^2 7 (fa and fb 2 each -> hypot 3 -> squared and rounded 7);
          two products 2                                            -> 17 |t1|
      t2: K2 6 (lambda 1, lambda^3 4, Cs product 1); u^4 13; product 1;
          the sums 2                                                -> 22 |t2|
      ps: the sums                                                  ->  2 |ps|
      cos(2 angle): angle rounded once (u |angle|), doubled, cosf 1 u:
          |K1| u^2 |dU - dV| d / 2 (2 |angle| + 1)
    |d ctf / d ki| <= hypot(w1, w2) = 1, and sinf / cosf (2 u each), w1 (2 u),
    the two products and the sum (3 u) on |w1 sin| + |w2 cos| <= 1.42 add 8 u."""
    a = np.asarray(attr, np.float32).astype(np.float64)
    ps_, volt, dU, dV, theta, Cs, ampC, phs = a
    d = np.asarray(d, np.float64)[:, None]
    ic = np.asarray(iCol, np.float64)[None, :]
    ir = np.asarray(iRow, np.float64)[None, :]
    lam = 12.2643247 / np.sqrt(volt * (1 + volt * 0.978466e-6))
    w1 = np.sqrt(1 - ampC * ampC)
    K1 = np.pi * lam
    K2 = np.pi / 2 * Cs * lam ** 3
    u2 = (ic / (ps_ * N)) ** 2 + (ir / (ps_ * N)) ** 2
    angle = np.arctan2(ir, ic) - theta
    defocus = -(dU * d + dV * d + (dU * d - dV * d) * np.cos(2 * angle)) / 2
    t1, t2 = K1 * defocus * u2, K2 * u2 * u2
    ki = t1 + t2 - phs
    ctf = -w1 * np.sin(ki) + ampC * np.cos(ki)
    dki = (17 * np.abs(t1) + 22 * np.abs(t2) + 2 * abs(phs) +
           abs(K1) * u2 * np.abs(dU - dV) * np.abs(d) / 2 * (2 * np.abs(angle) + 1))
    return ctf, U32 * (dki + 8)


class Scatter:
    """F, T (float64, flat), O, cnt, the tap count n per voxel and the budget's parts."""

    def __init__(self, size):
        self.F = np.zeros(size, np.complex128)
        self.T = np.zeros(size, np.float64)
        self.n = np.zeros(size, np.int64)
        self.aF = np.zeros(size)      # sum |val| (3 + 10 wt) (+ the CTF-search term)
        self.pF = np.zeros(size)      # sum |val| wt 4 theta
        self.sF = np.zeros(size)      # sum |val| wt
        self.aT = np.zeros(size)
        self.sT = np.zeros(size)
        self.O = np.zeros(3)
        self.cnt = 0
        self.vmaxF = 0.0              # largest |entry| of the binned deposit, F (re, im) / T
        self.vmaxT = 0.0

    @property
    def support(self):
        return self.n > 0

    def bF(self, P, binned=False):
        b = U32 * (self.aF + P * self.pF + self.n * self.sF)
        return b + self.n * 2.0 ** -47 * self.vmaxF if binned else b

    def bT(self, binned=False):
        b = U32 * (self.aT + self.n * self.sT)
        return b + self.n * 2.0 ** -47 * self.vmaxT if binned else b


def image_taps(vdim, pf, dat, ctf, quat, trans, off, w, px, N, l, nM, attr=None, nD=None):
    """Image l's first nM samples, every array [nM, nPxl] (idx / wt [8, nM, nPxl]):
    the fold flag, the 8 tap indices and weights, the cell corner, the
    (conjugated where folded) value and tv, and the budget's ingredients."""
    iCol, iRow = np.asarray(px.iCol), np.asarray(px.iRow)
    mat = _mats(quat[l, :nM])
    x, y, z = coords_f32(mat, iCol, iRow, pf)
    conj, idx, wt, corner = fold_taps(x, y, z, vdim)
    dx = (trans[l, :nM, 0] - off[l, 0])[:, None]
    dy = (trans[l, :nM, 1] - off[l, 1])[:, None]
    phase = np.exp(2j * np.pi * (iCol[None, :] * dx + iRow[None, :] * dy) / N)
    theta = 2 * np.pi * (np.abs(iCol[None, :] * dx) + np.abs(iRow[None, :] * dy)) / N
    wl = float(np.float32(w[l]))
    d = np.asarray(dat[l], np.complex64).astype(np.complex128)[None, :]
    if attr is None:
        c = np.asarray(ctf[l], np.float32).astype(np.float64)[None, :]
        dc = 0.0
    else:
        c, dc = ctf_f64(attr[l], np.asarray(nD, np.float64)[l, :nM], iCol, iRow, N)
    val = d * phase * c * wl
    val = np.where(conj, np.conj(val), val)
    return dict(mat=mat, coord=(x, y, z), conj=conj, idx=idx, wt=wt, corner=corner, val=val,
                tv=c * c * wl + np.zeros_like(theta), theta=theta, dx=dx, dy=dy,
                eF=np.abs(d) * wl * dc / U32,           # CTF search: the FP32 CTF's absolute error,
                eT=(2 * np.abs(c) + dc) * dc * wl / U32)   # in units of u like the other terms


def insert_f64(vdim, pf, dat, ctf, quat, trans, off, w, px, N, nC=None, attr=None, nD=None):
    """The float64 insert of dat [nImg, nPxl] under quat [nImg, mReco, 4],
    trans [nImg, mReco, 2], off [nImg, 2], w [nImg]; nC [nImg]: image l inserts
    its first min(nC[l], mReco) samples.  ctf [nImg, nPxl], or attr [nImg, 8]
    with nD [nImg, mReco] (ctf=None) for the CTF-search insert."""
    quat = np.asarray(quat, np.float64)
    trans = np.asarray(trans, np.float64)
    off = np.asarray(off, np.float64)
    nImg, mReco = quat.shape[:2]
    iCol = np.asarray(px.iCol)
    out = Scatter((vdim // 2 + 1) * vdim * vdim)
    for l in range(nImg):
        nM = mReco if nC is None else max(0, min(int(nC[l]), mReco))
        if nM == 0:
            continue
        t = image_taps(vdim, pf, dat, ctf, quat, trans, off, w, px, N, l, nM, attr, nD)
        mat, idx, wt, val, tv, theta, dx, dy = (t[k] for k in ("mat", "idx", "wt", "val", "tv", "theta",
                                                               "dx", "dy"))
        av, eF, eT = np.abs(val), t["eF"], t["eT"]
        for k in range(8):
            np.add.at(out.F, idx[k], val * wt[k])
            np.add.at(out.T, idx[k], tv * wt[k])
            np.add.at(out.n, idx[k], 1)
            np.add.at(out.aF, idx[k], av * (3 + 10 * wt[k]) + eF * wt[k])
            np.add.at(out.pF, idx[k], av * wt[k] * 4 * theta)
            np.add.at(out.sF, idx[k], av * wt[k])
            np.add.at(out.aT, idx[k], tv * (3 + 10 * wt[k]) + eT * wt[k])
            np.add.at(out.sT, idx[k], tv * wt[k])
        out.O -= np.array([np.sum(mat[:, a] * dx[:, 0] + mat[:, 3 + a] * dy[:, 0]) for a in range(3)])
        out.cnt += nM
        # the binned deposit's entries: one per (distinct rotation, pixel), members summed
        _, inv = np.unique(quat[l, :nM].view(np.uint64).reshape(nM, 4), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        gv = np.zeros((inv.max() + 1, len(iCol)), np.complex128)
        gt = np.zeros((inv.max() + 1, len(iCol)))
        np.add.at(gv, inv, val)
        np.add.at(gt, inv, tv)
        fin = np.isfinite(gv)
        if fin.any():
            out.vmaxF = max(out.vmaxF, np.abs(gv.real[fin]).max(), np.abs(gv.imag[fin]).max())
        out.vmaxT = max(out.vmaxT, gt.max())
    return out


def project_f64(vol, vdim, pf, mat, px):
    """Volume::getByInterpolationFT at R (iCol pf, iRow pf, 0) for mat [nR, 9]
    (column-major): (P [nR, nPxl] complex128, budget [nR, nPxl]).  Per pixel,
    over its 8 taps: b = u [ sum |V| (3 + 10 wt) + 8 sum |V| wt ] -- the
    weight factors' absolute error, the relative roundings of the weight and
    value products, and the 8-term FP32 sum."""
    mat = np.asarray(mat, np.float64).reshape(-1, 9)
    x, y, z = coords_f32(mat, px.iCol, px.iRow, pf)
    conj, idx, wt, _ = fold_taps(x, y, z, vdim)
    V = np.asarray(vol, np.complex64).astype(np.complex128).reshape(-1)[idx]      # [8, nR, nPxl]
    P = (V * wt).sum(0)
    aV = np.abs(V)
    b = U32 * ((aV * (3 + 10 * wt)).sum(0) + 8 * (aV * wt).sum(0))
    return np.where(conj, np.conj(P), P), b


def worst(got, ref, budget, mask=None):
    """Largest |got - ref| / budget over the voxels of mask (default: all); a
    voxel with no budget must be exact."""
    m = np.ones(ref.shape, bool) if mask is None else mask
    if not m.any():
        return 0.0
    err, b = np.abs(got[m] - ref[m]), budget[m]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def check_insert(gF, gT, ref, P, binned=False, skip=None):
    """Assert the per-voxel check of an insert's F (complex, flat) and T against
    ``ref`` (a Scatter): every voxel within its budget, exactly 0 outside the
    reference's support; skip: voxels left out (the non-finite ones).  Returns
    the largest err / budget of (F.re, F.im, T)."""
    sup = ref.support
    assert not gF[~sup].any() and not gT[~sup].any(), "non-zero voxel outside the reference's support"
    m = sup if skip is None else sup & ~skip
    bF, bT = ref.bF(P, binned), ref.bT(binned)
    r = (worst(gF.real, ref.F.real, bF, m), worst(gF.imag, ref.F.imag, bF, m), worst(gT, ref.T, bT, m))
    assert max(r) <= 1, f"largest err / budget (F.re, F.im, T) = {r}"
    return r
