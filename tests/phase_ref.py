"""Float64 reference of the 3D local phase and its per-sample error budget.

Pure numpy; takes the arrays exactly as thx_local_phase* gets them: vol
complex64 half-complex [vdim, vdim, vdim/2+1] (index z, y, x) or [nK, ...]
with cls [nImg]; quat [nImg, nR, 4] and trans [nImg, nT, 2] float64; dat
[nImg, nPxl] complex64, ctf and sig (sigRcp) [nImg, nPxl] float32 -- ctfD
[nImg, nD, nPxl] for the CTF search --; iCol, iRow [nPxl] int, idim, pf.

project64   Projector::project (src/Projector.cpp:365-368) on
            Volume::getByInterpolationFT (src/Image/Volume.cpp:314-338): the
            first two columns of rotate3D's matrix (src/Geometry/Euler.cpp:
            181-189), (x, y, z) = R (pf iCol, pf iRow, 0); conjHalf
            (include/Image/Volume.h:135-147) folds with conj = !(x >= 0),
            negating all three; floor, rows and slices wrapped into [0, vdim),
            the eight weights of WG_TRI_INTERP_LINEAR
            (include/Functions/Interpolation.h:187-200), the sum conjugated
            where the sample was folded.  As local.hip's header and
            common.h::interp_ft state it, all in float64 (the coordinates are
            NOT rounded to FP32: that rounding is a term of the budget).
dvp64       sum_i s |d - c T P|^2, T = exp(-2 pi i (iCol tx + iRow ty) / idim)
            (translate(), src/Image/ImageFunctions.cpp:233-252).
weights64   src/Optimiser.cpp:1383-1402 at the final baseline, nC = 1.

The budget ("The local phase's per-sample budget"), with
u = 2^-24, Pa = sum_taps w |v| >= |P| (the magnitude the tap sum's roundings
are relative to) and per sample
    S_A = sum |s| |d|^2,  S_B = sum |s| c^2 Pa^2,  S_X = sum 2 |s| |c| |d| Pa,
    S = S_A + S_B + S_X,
is absolute (no floor relative to |dvp|):
    u [ S (nPxl + K_LOC) + nPxl S_X + C ] + 4 P_HW u H
  nPxl S   FP32 accumulation of the nPxl terms of A, of B and of X, any order
  nPxl S_X the X sum is a K = 2 nPxl product (P.re U + P.im V: two chained
           FMAs of the FP32 MFMA per pixel), one more rounding per pixel
  K_LOC    the roundings that form one term, below
  C        the coordinates are rounded to FP32 before floor: each moves by
           <= u |coordinate|, P by <= u (|x| + |y| + |z|) D with D the largest
           difference along an edge of the cell (trilinear interpolation is
           continuous across cells and, on a Hermitian x = 0 plane, across the
           fold), and the sample by sum |s| (2 c^2 Pa + 2 |c| |d|) times that
  H        the phase: trans is cast to FP32, divided by idim, multiplied by
           iCol and iRow and added -- four roundings of magnitude
           theta = 2 pi (|iCol tx| + |iRow ty|) / idim -- then the hardware
           sin / cos of revolutions, P_HW = 4 behind that (the project's rule
           for every phase_shift output, scatter_ref.py); T moves by
           <= 4 P_HW u theta, the sample by sum 2 |s| |c| |d| Pa theta times it
"""
import numpy as np

U = 2.0 ** -24
P_HW = 4.0

# K_LOC, counted from k_local_fused (local.hip), interp_ft (common.h) and the
# gathers of the other layouts, in units of u times the term's share of S.
# The three kinds of term never share a pixel's share of S, so the count of
# one term is the largest of the three, plus the two bias adds.
#   P       1 - dx (dx = x - floor x is exact), the two products of a weight:
#           3 u relative per weight; tap times weight 1; the sum of eight
#           taps 7 (the quad / pair trees of the cell and y-pair layouts take
#           fewer): |delta P| <= 11 u Pa per component sum, and in modulus
#   A term  s (dx^2 + dy^2): one u between the squares, the add, times s       3
#   B term  b (px^2 + py^2), b = s c c: 2; the squares and their add 2; the
#           product 1; |P|^2 moves by 2 Pa |delta P| = 22 u Pa^2              27
#   X term  P.re U + P.im V, Y = (-2 s c) d: s c and the product with d, 2 u
#           on each component of Y; U = Yr Tx + Yi Ty (V alike): two products
#           and an add, 2 u (|Yr Tx| + |Yi Ty|) <= 2 u |Y| per component,
#           2 sqrt 2 u |Y| in modulus of (U, V); P's 11; the products with P
#           are exact (FMA), their accumulation is in the nPxl parts
#           2 + 2.83 + 11                                            15.83 -> 16
#           CTF search: b P.re^2 and b P.im^2 enter the same accumulator (two
#           more chained FMAs per pixel, inside nPxl S: S_B's nPxl adds were
#           the bias sum's), the squares round once each                 B: 27
#   bias    (A + B) and + X: one rounding each of a value <= S                 2
K_LOC = 27 + 2


# ------------------------------------------------------------------ geometry
def rot2(quat):
    """First two columns of rotate3D(q) = I + 2 q0 A + 2 A A, A = [[0, -q3, q2],
    [q3, 0, -q1], [-q2, q1, 0]], in quat_to_mat's order of operations:
    [..., 6] = (R00, R10, R20, R01, R11, R21)."""
    q = np.asarray(quat, np.float64)
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    z = np.zeros_like(q0)
    A = [[z, -q3, q2], [q3, z, -q1], [-q2, q1, z]]
    m = []
    for c in range(2):
        for r in range(3):
            aa = z
            for k in range(3):
                aa = aa + (2 * A[r][k]) * A[k][c]
            m.append((1.0 if r == c else 0.0) + (2 * q0) * A[r][c] + aa)
    return np.stack(m, -1)


def coords64(quat, iCol, iRow, pf):
    """(x, y, z) [..., nPxl] float64 of R (pf iCol, pf iRow, 0)."""
    m = rot2(quat)[..., None]
    X = (np.asarray(iCol, np.int64) * pf).astype(np.float64)
    Y = (np.asarray(iRow, np.int64) * pf).astype(np.float64)
    return m[..., 0, :] * X + m[..., 3, :] * Y, m[..., 1, :] * X + m[..., 4, :] * Y, \
        m[..., 2, :] * X + m[..., 5, :] * Y


BOX = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]    # getFTHalf's order
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]


def cell(x, y, z):
    """Fold and floor: conj, the base (x0, y0, z0) int64 and the fractions."""
    conj = ~(x >= 0)
    sg = np.where(conj, -1.0, 1.0).astype(x.dtype)
    c = [x * sg, y * sg, z * sg]
    f = [np.floor(a) for a in c]
    return conj, [a.astype(np.int64) for a in f], [a - b for a, b in zip(c, f)]


def interp(vol, x, y, z, mut=None, extras=False):
    """Trilinear gather of the half-complex vol [vdim, vdim, vdim/2+1] at the
    coordinates (any shape, any float type; the arithmetic stays in theirs,
    widened to at least float64 for float64 input).  mut: a deliberately wrong
    restatement (test_phase_ref.py): "noconj", "nowrap" (row y0 + 1 taken as
    wrap(y0) + 1 in memory order) or ("tap", k) (tap 0 of flat sample k read
    from the next cell in x).  extras: also Pa = sum w |v| and D, the largest
    difference along a cell edge."""
    vdim, nc = vol.shape[0], vol.shape[2]
    conj, (x0, y0, z0), (fx, fy, fz) = cell(x, y, z)
    assert x0.min() >= 0 and x0.max() + 1 < nc, "tap outside the half-complex row"
    assert min(y0.min(), z0.min()) >= -vdim // 2 - 1 and max(y0.max(), z0.max()) + 1 <= vdim // 2
    flat = vol.reshape(-1)
    one = fx.dtype.type(1)
    wx, wy, wz = (one - fx, fx), (one - fy, fy), (one - fz, fz)
    ctype = np.complex128 if fx.dtype == np.float64 else np.complex64
    P = np.zeros(x.shape, ctype)
    Pa = np.zeros(x.shape)
    taps = []
    for n, (dz, dy, dx) in enumerate(BOX):
        zi, yi, xi = np.mod(z0 + dz, vdim), np.mod(y0 + dy, vdim), x0 + dx
        if mut == "nowrap" and dy:
            yi = np.mod(y0, vdim) + 1
        if isinstance(mut, tuple) and mut[0] == "tap" and n == 0:
            xi = xi.copy()
            xi.reshape(-1)[mut[1]] += 1
        v = flat[((zi * vdim + yi) * nc + xi) % flat.size]
        w = wx[dx] * wy[dy] * wz[dz]
        if ctype is np.complex64:       # FP32, tap by tap in box order as interp_ft
            P = (P.real + v.real * w) + 1j * (P.imag + v.imag * w)
            P = P.astype(np.complex64)
        else:
            P = P + v * w
        if extras:
            Pa = Pa + np.abs(v) * w
            taps.append(v)
    if mut != "noconj":
        P = np.where(conj, np.conj(P), P)
    if not extras:
        return P
    D = np.max([np.abs(taps[a] - taps[b]) for a, b in EDGES], axis=0)
    return P, Pa, D


def _per_image(vol, cls, nImg):
    vol = np.asarray(vol)
    if vol.ndim == 3:
        return [vol] * nImg
    return [vol[int(cls[l])] for l in range(nImg)]


def project64(vol, quat, iCol, iRow, pf, cls=None, mut=None, extras=False):
    """P [nImg, nR, nPxl] complex128 (with extras: P, Pa, D, |x| + |y| + |z|)."""
    quat = np.asarray(quat, np.float64)
    vols = _per_image(vol, cls, quat.shape[0])
    out = []
    for l in range(quat.shape[0]):
        x, y, z = coords64(quat[l], iCol, iRow, pf)
        m = None if isinstance(mut, tuple) and l else mut        # ("tap", k): image 0 only
        r = interp(vols[l].astype(np.complex128), x, y, z, mut=m, extras=extras)
        out.append(r + (np.abs(x) + np.abs(y) + np.abs(z),) if extras else r)
    if extras:
        return tuple(np.stack([o[k] for o in out]) for k in range(4))
    return np.stack(out)


def project_full(vol, quat, iCol, iRow, pf):
    """The same projection by a second route: the half volume extended to the
    full Hermitian cube F(-k) = conj F(k), interpolated with no fold."""
    vol = np.asarray(vol).astype(np.complex128)
    vdim, nc = vol.shape[0], vol.shape[2]
    h = vdim // 2
    full = np.zeros((vdim, vdim, 2 * h + 1), np.complex128)     # x = -h .. h at index x + h
    full[:, :, h:] = vol
    neg = np.arange(vdim)
    mz, my = np.mod(-neg, vdim)[:, None, None], np.mod(-neg, vdim)[None, :, None]
    xs = np.arange(1, h + 1)[None, None, :]
    full[:, :, h - np.arange(1, h + 1)] = np.conj(vol[mz, my, xs])
    out = []
    for l in range(len(quat)):
        x, y, z = coords64(quat[l], iCol, iRow, pf)
        x0, y0, z0 = (np.floor(a).astype(np.int64) for a in (x, y, z))
        fx, fy, fz = x - x0, y - y0, z - z0
        P = 0
        for dz, dy, dx in BOX:
            w = (fx if dx else 1 - fx) * (fy if dy else 1 - fy) * (fz if dz else 1 - fz)
            P = P + w * full[np.mod(z0 + dz, vdim), np.mod(y0 + dy, vdim), x0 + dx + h]
        out.append(P)
    return np.stack(out)


def phases(trans, iCol, iRow, idim):
    """T [nImg, nT, nPxl] complex128 and theta = 2 pi (|iCol tx| + |iRow ty|) / idim."""
    t = np.asarray(trans, np.float64)
    ic, ir = np.asarray(iCol, np.float64), np.asarray(iRow, np.float64)
    a, b = t[..., :1] * ic, t[..., 1:] * ir
    return np.exp(-2j * np.pi * (a + b) / idim), 2 * np.pi * (np.abs(a) + np.abs(b)) / idim


def _ctf3(ctf):
    c = np.asarray(ctf, np.float64)
    return (c[:, None, :], False) if c.ndim == 2 else (c, True)


# ----------------------------------------------------------------- reference
def dvp64(vol, quat, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None, P=None):
    """[nImg, nR, nT] float64, or [nImg, nR, nT, nD] for ctf = ctfD."""
    if P is None:
        P = project64(vol, quat, iCol, iRow, pf, cls)
    T, _ = phases(trans, iCol, iRow, idim)
    c, search = _ctf3(ctf)
    d, s = np.asarray(dat).astype(np.complex128), np.asarray(sig, np.float64)
    nImg, nR, nT, nD = len(d), P.shape[1], T.shape[1], c.shape[1]
    out = np.empty((nImg, nR, nT, nD))
    for l in range(nImg):
        TP = T[l][None, :, :] * P[l][:, None, :]                          # [r, t, i]
        for k in range(nD):
            e = d[l] - c[l, k] * TP
            out[l, :, :, k] = (e.real ** 2 + e.imag ** 2) @ s[l]
    return out if search else out[..., 0]


def sums(vol, quat, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None):
    """dict of float64 arrays shaped like dvp64's result: the magnitude sums
    S_A, S_B, S_X, S and the sensitivities C (coordinate rounding) and H
    (phase) of the budget, in units of u and 4 P_HW u."""
    _, Pa, D, L1 = project64(vol, quat, iCol, iRow, pf, cls, extras=True)  # [l, r, i]
    _, th = phases(trans, iCol, iRow, idim)                                # [l, t, i]
    c, search = _ctf3(ctf)
    c = np.abs(c)
    d, s = np.abs(np.asarray(dat).astype(np.complex128)), np.abs(np.asarray(sig, np.float64))
    nImg, nR, nT, nD = len(d), Pa.shape[1], th.shape[1], c.shape[1]
    SA = np.broadcast_to((s * d ** 2).sum(1)[:, None, None, None], (nImg, nR, nT, nD)).copy()
    SB, SX, C, H = (np.empty((nImg, nR, nT, nD)) for _ in range(4))
    for l in range(nImg):
        for k in range(nD):
            b, y = s[l] * c[l, k] ** 2, 2 * s[l] * c[l, k] * d[l]
            SB[l, :, :, k] = (Pa[l] ** 2 @ b)[:, None]
            SX[l, :, :, k] = (Pa[l] @ y)[:, None]
            C[l, :, :, k] = ((L1[l] * D[l] * (2 * Pa[l] * b + y)).sum(1))[:, None]
            H[l, :, :, k] = np.einsum("ri,ti->rt", Pa[l] * y, th[l])
    r = dict(S_A=SA, S_B=SB, S_X=SX, S=SA + SB + SX, C=C, H=H)
    return r if search else {k: v[..., 0] for k, v in r.items()}


def budget(sm, nPxl):
    return U * (sm["S"] * (nPxl + K_LOC) + nPxl * sm["S_X"] + sm["C"]) + 4 * P_HW * U * sm["H"]


# ------------------------------------------------------------------- weights
def weights64(dvp, pC, pR, pT, pD=None):
    """src/Optimiser.cpp:1383-1402 at the final baseline with nC = 1: with
    e = exp(dvp - max), wC = sum e pR pT [pD] -- the weight of the image's one
    class carries the other three priors and no pC, as k_local_weights has it
    --, wR = pC sum_t e pT, wT = pC sum_r e pR[, wD = pC sum e pR pT].
    -> wC [nImg], wR [nImg, nR], wT [nImg, nT][, wD [nImg, nD]], base [nImg]."""
    d = np.asarray(dvp, np.float64)
    pC, pR, pT = (np.asarray(a, np.float64) for a in (pC, pR, pT))
    if pD is None:
        base = d.max(axis=(1, 2))
        e = np.exp(d - base[:, None, None])
        wR = pC[:, None] * np.einsum("lrt,lt->lr", e, pT)
        wT = pC[:, None] * np.einsum("lrt,lr->lt", e, pR)
        return np.einsum("lrt,lr,lt->l", e, pR, pT), wR, wT, base
    pD = np.asarray(pD, np.float64)
    base = d.max(axis=(1, 2, 3))
    e = np.exp(d - base[:, None, None, None])
    wR = pC[:, None] * np.einsum("lrtd,lt,ld->lr", e, pT, pD)
    wT = pC[:, None] * np.einsum("lrtd,lr,ld->lt", e, pR, pD)
    wD = pC[:, None] * np.einsum("lrtd,lr,lt->ld", e, pR, pT)
    return np.einsum("lrtd,lr,lt,ld->l", e, pR, pT, pD), wR, wT, wD, base


def weights_literal(dvp, pC, pR, pT, pD=None):
    """The same by the reference's own loop (running baseline, rescale by
    exp(old - new)), one image at a time."""
    d = np.asarray(dvp, np.float64)
    search = pD is not None
    if not search:
        d, pD = d[..., None], np.ones((len(d), 1))
    nImg, nR, nT, nD = d.shape
    wC, wR, wT, wD = np.zeros(nImg), np.zeros((nImg, nR)), np.zeros((nImg, nT)), np.zeros((nImg, nD))
    base = np.full(nImg, np.nan)
    for l in range(nImg):
        for r in range(nR):
            for t in range(nT):
                for k in range(nD):
                    w = d[l, r, t, k]
                    if base[l] != base[l]:
                        base[l] = w
                    if w > base[l]:
                        nf = np.exp(base[l] - w)
                        wC[l] *= nf
                        wR[l] *= nf
                        wT[l] *= nf
                        wD[l] *= nf
                        base[l] = w
                    s = np.exp(w - base[l])
                    wC[l] += s * (pR[l, r] * pT[l, t] * pD[l, k])
                    wR[l, r] += s * (pC[l] * pT[l, t] * pD[l, k])
                    wT[l, t] += s * (pC[l] * pR[l, r] * pD[l, k])
                    wD[l, k] += s * (pC[l] * pR[l, r] * pT[l, t])
    return (wC, wR, wT, wD, base) if search else (wC, wR, wT, base)


def worst(got, ref, bound):
    """Largest |got - ref| / bound; entries with bound 0 must match exactly
    (inf otherwise).  NaN in got counts as inf."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ----------------------------------------------------------------- emulation
def emu32(vol, quat, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None):
    """The kernel's sums in sequential FP32, operation by operation as
    k_local_fused writes them (set order, no contraction except the MFMA's
    fused multiply-adds): FP64 rotation rounded to FP32, interp_ft in FP32,
    Y, U, V, b in FP32 with phase_shift's FP32 argument (sin / cos of it taken
    in float64 and rounded), A, the bias and the K = 2 nPxl product each
    accumulated in turn, dvp = (A + B) + X."""
    f = np.float32
    quat = np.asarray(quat, np.float64)
    nImg = quat.shape[0]
    vols = _per_image(vol, cls, nImg)
    c3, search = _ctf3(ctf)
    c3 = c3.astype(f)
    ic, ir = np.asarray(iCol, np.int64), np.asarray(iRow, np.int64)
    t32 = np.asarray(trans, np.float64).astype(f) / f(idim)               # [l, t, 2]
    rev = -(ic.astype(f) * t32[..., :1] + ir.astype(f) * t32[..., 1:])    # [l, t, i] FP32
    fr = (rev - np.rint(rev)).astype(np.float64)
    Tx, Ty = np.cos(2 * np.pi * fr).astype(f), np.sin(2 * np.pi * fr).astype(f)
    d, s = np.asarray(dat), np.asarray(sig, f)
    dr, di = d.real.astype(f), d.imag.astype(f)
    nR, nT, nD, nPxl = quat.shape[1], t32.shape[1], c3.shape[1], len(ic)
    out = np.empty((nImg, nR, nT, nD), f)
    fma = lambda a, b, acc: (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(f)
    for l in range(nImg):
        x, y, z = (a.astype(f) for a in coords64(quat[l], iCol, iRow, pf))
        P = interp(vols[l].astype(np.complex64), x, y, z)                 # [r, i] complex64
        pr, pi = P.real.astype(f), P.imag.astype(f)
        A, bias = f(0), np.zeros(nR, f)
        X = np.zeros((nR, nT, nD), f)
        for i in range(nPxl):
            A = A + s[l, i] * (dr[l, i] * dr[l, i] + di[l, i] * di[l, i])
            cv = c3[l, :, i]                                              # [nD]
            k2 = f(-2) * s[l, i] * cv
            yr, yi = k2 * dr[l, i], k2 * di[l, i]
            Uv = yr[None, :] * Tx[l, :, i, None] + yi[None, :] * Ty[l, :, i, None]     # [t, d]
            Vv = yi[None, :] * Tx[l, :, i, None] - yr[None, :] * Ty[l, :, i, None]
            X = fma(pr[:, i, None, None], Uv[None], X)
            X = fma(pi[:, i, None, None], Vv[None], X)
            b = s[l, i] * cv * cv
            if search:
                X = fma((pr[:, i] * pr[:, i])[:, None, None], b[None, None, :], X)
                X = fma((pi[:, i] * pi[:, i])[:, None, None], b[None, None, :], X)
            else:
                bias = bias + b[0] * (pr[:, i] * pr[:, i] + pi[:, i] * pi[:, i])
        out[l] = (A + bias)[:, None, None] + X
    return out if search else out[..., 0]
