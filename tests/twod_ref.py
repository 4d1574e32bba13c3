"""Float64 reference of the 2D classification kernels (csrc/twod.hip) and
their absolute error budgets.

Pure numpy; takes the arrays exactly as the entry points get them: img
complex64 half-complex [vdim, vdim/2+1] (index row, column; negative rows
wrapped) or [nK, ...] with cls [nImg]; rot [..., 2] float64 (cos, sin); trans
[nImg, nT, 2] float64; dat [nImg, nPxl] complex64, ctf and sig (sigRcp)
[nImg, nPxl] float32 -- ctfD [nImg, nD, nPxl] for the CTF search --; iCol,
iRow [nPxl] int, idim, pf.

project2d_64  Image::getByInterpolationFT: (x, y) = R (pf iCol, pf iRow),
              R = [[c, -s], [s, c]]; conjugate when !(x >= 0), negating both;
              floor, rows wrapped into [0, vdim); the four weights of
              WG_BI_INTERP_LINEAR.  All in float64: the coordinates are NOT
              rounded to FP32, that rounding is a term of the budget.
dvp2d_64      sum_i s |d - c T P|^2 with phase_ref.phases' T; with ctfD the
              columns are ordered t nD + d.
insert2d_64   insertP(dmat22) / Image::addFT: the coordinate formed in FP64
              and rounded to FP32 (the kernel's fold and floor decisions), the
              rest in float64: F += dat phase(+) ctf w, T += ctf^2 w, the value
              conjugated on fold, 4 taps (np.add.at); per class
              O[k] += -R (t - off), counter[k] += 1.

Budgets, all absolute (no floor relative to a maximum), u = 2^-24, counted
from twod.hip.

The gather (interp2), per output, in modulus, Pa = sum_taps w |v|:
    bP = u [ K_GATHER Pa + (|x| + |y|) D ]
  K_GATHER 1 - dx and 1 - dy round once each (dx = x - floor x is exact), their
           product once: 3 u relative per weight; tap times weight 1; the sum
           of four taps 3 (the first add to 0 is exact)                      7
  (|x| + |y|) D   rot2 rounds each coordinate to FP32 before the floor, so it
           moves by <= u |coordinate| and P by <= u (|x| + |y|) D, D the
           largest difference along an edge of the cell (bilinear
           interpolation is continuous across cells and, on a Hermitian x = 0
           column, across the fold)

The likelihood (k_local2d, the direct form), per sample, with
g = |d| + |c| Pa per pixel and
    S = sum |s| g^2,   S_P = sum 2 |s| g |c| Pa,
    C = sum 2 |s| g |c| (|x| + |y|) D,   H = sum 2 |s| g |c| Pa theta:
    u [ S (n_acc + K_DIR) + (K_GATHER + 1) S_P + C ] + 4 P_HW u H
  n_acc    ceil(nPxl / 256) terms per thread, the 6 steps of wave_sum, 3 adds
           across the four waves (the first add to 0 is exact)
  K_DIR    scan_ref.K_DIR = 14, the same operations: cmul(T, P) two products
           and an add per component, times c, d minus that, er^2 + ei^2,
           times s
  K_GATHER + 1   P carries the gather's 7 u Pa; the hardware sin and cos
           round T once more (u |T|): the error e = d - c T P moves by
           <= 8 u |c| Pa, |e|^2 by 2 g times that
  C        the coordinate term of the gather, through 2 g |c|
  H        the phase: trans cast to FP32, divided by idim, multiplied by iCol
           and iRow and added, four roundings of magnitude theta, then the
           hardware sin / cos of revolutions with the margin P_HW = 4 (the
           project's rule for every phase_shift output)

The marginals: weights2d_bounds, the per-image form of scan_ref.weight_bounds:
every term e p moves by at most expm1(b_sample + b_top) of itself, plus 1e-4
of the reference for the FP32 exponential and the sums.

The insert (k_insert2d, scatter2): scatter_ref's per-voxel form
    b_v = u [ sum |val| (2 + wt (10 + 4 P theta)) + n_v sum |val| wt ]
  2        two weight factors, each off by <= u in absolute terms
  10       as scatter_ref (the complex product, the CTF and w products, the
           weight product, the tap product)
  n_v      FP32 atomics: the n_v taps of the voxel summed in any order
  the CTF-search variant adds scatter_ref.ctf_f64's absolute CTF term.
O: double atomics in any order, per class and component
    (n_k + 3) 2^-53 sum (|c dx| + |s dy|)
  n_k samples of the class summed in any order, and the three roundings that
  form one term (t - off, the two products and their difference; the device
  may fuse one product).  counter: exact.
"""
from fractions import Fraction

import numpy as np

import phase_ref as PR
import scan_ref as SR
import scatter_ref as SC

U = 2.0 ** -24
P_HW = PR.P_HW
K_GATHER = 7
K_DIR = SR.K_DIR
THREADS = 256          # L2D_THREADS
TMAX = 16              # L2D_TMAX


def worst(got, ref, bound):
    """phase_ref.worst for real or complex values (the error in modulus)."""
    g = np.asarray(got)
    g = g.astype(np.complex128 if np.iscomplexobj(g) or np.iscomplexobj(ref) else np.float64)
    err = np.abs(g - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------ geometry
def coords2_64(rot, iCol, iRow, pf):
    """(x, y) [..., nPxl] float64 of R (pf iCol, pf iRow), every product and
    sum rounded on its own."""
    r = np.asarray(rot, np.float64)
    X = (np.asarray(iCol, np.int64) * pf).astype(np.float64)
    Y = (np.asarray(iRow, np.int64) * pf).astype(np.float64)
    c, s = r[..., :1], r[..., 1:]
    return c * X - s * Y, s * X + c * Y


def _fused(a, b, c, d, sign):
    """The two fused forms of a b + sign c d in exact rationals, rounded once
    more to float64: fma(a, b, sign (c d)) and fma(sign c, d, (a b))."""
    fa, fb, fc, fd = Fraction(a), Fraction(b), Fraction(c), Fraction(d)
    return (float(fa * fb + sign * Fraction(c * d)), float(Fraction(a * b) + sign * fc * fd))


def fused_agree(rot, iCol, iRow, pf):
    """Per rotation [...]: fold, floor and the FP32-rounded coordinate of every
    sample are the same whether rot2's FP64 expression rounds each product or
    is contracted into a fused multiply-add (either product).  A sample whose
    FP32 rounding is the same over the whole interval of width
    2^-51 (|c X| + |s Y|) about the unfused value passes at once; the others
    (exact grid points, as a rule) are evaluated in exact rationals."""
    r = np.asarray(rot, np.float64)
    lead = r.shape[:-1]
    r = r.reshape(-1, 2)
    X = (np.asarray(iCol, np.int64) * pf).astype(np.float64)
    Y = (np.asarray(iRow, np.int64) * pf).astype(np.float64)
    ok = np.ones(len(r), bool)
    for q, (c, s) in enumerate(r):
        for a, b, sign in ((c * X, s * Y, -1.0), (s * X, c * Y, 1.0)):
            v = a + sign * b
            dl = 2.0 ** -51 * (np.abs(a) + np.abs(b))
            lo, hi = (v - dl).astype(np.float32), (v + dl).astype(np.float32)
            for i in np.flatnonzero((lo != hi) | (np.signbit(lo) != np.signbit(hi))):
                first, second = (c, s) if sign < 0 else (s, c)
                want = np.float32(v[i])
                for f in _fused(first, X[i], second, Y[i], int(sign)):
                    g = np.float32(f)
                    if g != want or (g >= 0) != (want >= 0):
                        ok[q] = False
    return ok.reshape(lead)


def cell2(x, y):
    """Fold and floor: conj, the base (x0, y0) int64 and the fractions."""
    conj = ~(x >= 0)
    sg = np.where(conj, -1.0, 1.0).astype(x.dtype)
    c = [x * sg, y * sg]
    f = [np.floor(a) for a in c]
    return conj, [a.astype(np.int64) for a in f], [a - b for a, b in zip(c, f)]


def taps_in_range(x, y, vdim):
    """Every tap of every sample inside the half-complex image."""
    _, (x0, y0), _ = cell2(x, y)
    return bool(x0.min() >= 0 and x0.max() + 1 <= vdim // 2 and y0.min() >= -(vdim // 2)
                and y0.max() + 1 <= vdim // 2)


BOX2 = [(dy, dx) for dy in (0, 1) for dx in (0, 1)]             # getFTHalf's order j, i
EDGES2 = [(0, 1), (2, 3), (0, 2), (1, 3)]


def interp2(img, x, y, mut=None, extras=False):
    """Bilinear gather of the half-complex img [vdim, vdim/2+1] at the
    coordinates (any shape; float64, or float32 for interp2's own order of
    operations with every product and sum rounded).  mut, a deliberately wrong
    restatement (test_twod_ref.py): "noconj", "foldgt" (fold decided by
    x > 0), "nowrap" (row y0 + 1 taken as wrap(y0) + 1 in memory order: past the
    image, read as 0, when y0 = -1),
    "tap11" (tap (1, 1) read from the next cell in x).  extras: also
    Pa = sum w |v| and D, the largest difference along a cell edge."""
    vdim, nc = img.shape
    if mut == "foldgt":
        conj = ~(x > 0)
        sg = np.where(conj, -1.0, 1.0).astype(x.dtype)
        xs, ys = x * sg, y * sg
        fxs, fys = np.floor(xs), np.floor(ys)
        (x0, y0), (fx, fy) = (fxs.astype(np.int64), fys.astype(np.int64)), (xs - fxs, ys - fys)
    else:
        conj, (x0, y0), (fx, fy) = cell2(x, y)
    assert x0.min() >= 0 and x0.max() + 1 < nc, "tap outside the half-complex row"
    assert y0.min() >= -(vdim // 2) and y0.max() + 1 <= vdim // 2, "row outside the box"
    flat = img.reshape(-1)
    one = fx.dtype.type(1)
    wx, wy = (one - fx, fx), (one - fy, fy)
    f32 = fx.dtype == np.float32
    re, im = np.zeros(x.shape, fx.dtype), np.zeros(x.shape, fx.dtype)
    Pa, taps = np.zeros(x.shape), []
    for dy, dx in BOX2:
        yi, xi = np.mod(y0 + dy, vdim), x0 + dx
        if mut == "nowrap" and dy:
            yi = np.mod(y0, vdim) + 1
        if mut == "tap11" and dy and dx:
            xi = xi + 1
        v = flat[(yi * nc + xi) % flat.size]
        if mut == "nowrap" and dy:
            v = np.where(yi == vdim, 0, v)          # past the image's last row
        w = wx[dx] * wy[dy]
        if f32:
            re, im = re + v.real.astype(np.float32) * w, im + v.imag.astype(np.float32) * w
        else:
            re, im = re + v.real * w, im + v.imag * w
        if extras:
            Pa = Pa + np.abs(v) * w
            taps.append(v)
    P = re + 1j * np.where(conj & (mut != "noconj"), -im, im)
    P = P.astype(np.complex64) if f32 else P
    if not extras:
        return P
    D = np.max([np.abs(taps[a] - taps[b]) for a, b in EDGES2], axis=0)
    return P, Pa, D


def _per_image(img, cls, nImg, mut=None):
    img = np.asarray(img)
    if img.ndim == 2:
        return [img] * nImg
    if cls is None:
        return [img[0]] * nImg
    return [img[int(cls[0 if mut == "cls0" else l])] for l in range(nImg)]


def project2d_64(img, rot, iCol, iRow, pf, cls=None, mut=None, extras=False):
    """rot [nR, 2] with img [vdim, nc] -> P [nR, nPxl] complex128; rot
    [nImg, nR, 2] (img [nK, ...] with cls) -> [nImg, nR, nPxl].  With extras:
    (P, Pa, D, |x| + |y|)."""
    rot = np.asarray(rot, np.float64)
    single = rot.ndim == 2
    rot3 = rot[None] if single else rot
    imgs = _per_image(img, cls, len(rot3), mut)
    gm = None if mut == "cls0" else mut
    out = []
    for l in range(len(rot3)):
        x, y = coords2_64(rot3[l], iCol, iRow, pf)
        r = interp2(imgs[l].astype(np.complex128), x, y, mut=gm, extras=extras)
        out.append(r + (np.abs(x) + np.abs(y),) if extras else r)
    if extras:
        res = tuple(np.stack([o[k] for o in out]) for k in range(4))
        return tuple(a[0] for a in res) if single else res
    return out[0] if single else np.stack(out)


def gather_budget(Pa, D, L1):
    return U * (K_GATHER * Pa + L1 * D)


def emu_project2d_32(img, rot, iCol, iRow, pf):
    """k_project2d as interp2 (twod.hip) writes it: the FP64 rotation rounded
    to FP32, then every product and sum in FP32, taps in box order."""
    x, y = coords2_64(rot, iCol, iRow, pf)
    return interp2(np.asarray(img, np.complex64), x.astype(np.float32), y.astype(np.float32))


# ---------------------------------------------------------------- likelihood
def _ctf3(ctf):
    c = np.asarray(ctf, np.float64)
    return (c[:, None, :], False) if c.ndim == 2 else (c, True)


def dvp2d_64(img, rot, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None, P=None, mut=None):
    """[nImg, nR, nT] float64, or [nImg, nR, nT nD] (column t nD + d) for
    ctf = ctfD.  mut: "droplast", "drop256", "droplastcol", "colorder",
    "ctfd0", "cls0", "transsign", or one of interp2's."""
    gm = mut if mut in ("noconj", "foldgt", "nowrap", "tap11", "cls0") else None
    if P is None or gm:
        P = project2d_64(img, rot, iCol, iRow, pf, cls, mut=gm)
    tr = np.asarray(trans, np.float64)
    T, _ = PR.phases(-tr if mut == "transsign" else tr, iCol, iRow, idim)
    c, search = _ctf3(ctf)
    d, s = np.asarray(dat).astype(np.complex128), np.asarray(sig, np.float64).copy()
    nImg, nR, nT, nD, nPxl = len(d), P.shape[1], T.shape[1], c.shape[1], d.shape[1]
    if mut == "droplast":
        s[:, -1] = 0
    if mut == "drop256" and nPxl > 256:
        s[:, 256] = 0
    out = np.empty((nImg, nR, nT, nD))
    for l in range(nImg):
        TP = T[l][None, :, :] * P[l][:, None, :]                          # [r, t, i]
        for k in range(nD):
            e = d[l] - c[l, 0 if mut == "ctfd0" else k] * TP
            out[l, :, :, k] = (e.real ** 2 + e.imag ** 2) @ s[l]
    if mut == "colorder":
        out = out.transpose(0, 1, 3, 2)
    out = np.ascontiguousarray(out).reshape(nImg, nR, nT * nD)
    if mut == "droplastcol":
        out[:, :, 2 * TMAX - 1::TMAX] = np.nan         # the last column of every pass after the first
        if nT * nD > TMAX and (nT * nD) % TMAX:
            out[:, :, -1] = np.nan
    return out


def sums2d(img, rot, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None):
    """dict of [nImg, nR, nT nD] float64 arrays: S, S_P, C, H of the budget."""
    _, Pa, D, L1 = project2d_64(img, rot, iCol, iRow, pf, cls, extras=True)     # [l, r, i]
    _, th = PR.phases(trans, iCol, iRow, idim)                                 # [l, t, i]
    c, _ = _ctf3(ctf)
    c = np.abs(c)
    d, s = np.abs(np.asarray(dat).astype(np.complex128)), np.abs(np.asarray(sig, np.float64))
    nImg, nR, nT, nD = len(d), Pa.shape[1], th.shape[1], c.shape[1]
    S, SP, C, H = (np.empty((nImg, nR, nT, nD)) for _ in range(4))
    for l in range(nImg):
        for k in range(nD):
            g = d[l] + c[l, k] * Pa[l]                                       # [r, i]
            y = 2 * s[l] * g * c[l, k]
            S[l, :, :, k] = ((s[l] * g ** 2).sum(1))[:, None]
            SP[l, :, :, k] = ((y * Pa[l]).sum(1))[:, None]
            C[l, :, :, k] = ((y * L1[l] * D[l]).sum(1))[:, None]
            H[l, :, :, k] = np.einsum("ri,ti->rt", y * Pa[l], th[l])
    return {k: v.reshape(nImg, nR, nT * nD) for k, v in dict(S=S, S_P=SP, C=C, H=H).items()}


def n_acc(nPxl):
    return -(-nPxl // THREADS) + 6 + 3


def dvp_budget(sm, nPxl):
    return U * (sm["S"] * (n_acc(nPxl) + K_DIR) + (K_GATHER + 1) * sm["S_P"] + sm["C"]) + \
        4 * P_HW * U * sm["H"]


def scan_input_budget(sm):
    """What the 2D global scan's operands add to the scan's own budget: rotP
    is thx_project2d's output (the gather's K_GATHER u Pa and its coordinate
    term) rounded to FP32 (1), traP the phase table (the phase term and one
    rounding of T)."""
    return U * ((K_GATHER + 2) * sm["S_P"] + sm["C"]) + 4 * P_HW * U * sm["H"]


# ------------------------------------------------------------------- weights
def _dvp4(dvp, nT, pD):
    d = np.asarray(dvp, np.float64)
    return d.reshape(d.shape[0], d.shape[1], nT, -1) if pD is not None else d


def weights2d_64(dvp, pC, pR, pT, pD=None):
    """phase_ref.weights64 of dvp [nImg, nR, nT nD]."""
    return PR.weights64(_dvp4(dvp, np.shape(pT)[1], pD), pC, pR, pT, pD)


def weights2d_bounds(dvp, bud, pC, pR, pT, pD=None):
    """Per-entry bounds of the marginals of a kernel whose dvp may differ from
    dvp by bud per sample: scan_ref.weight_bounds per image (each term e p
    moves by at most expm1(b_sample + b_top) of itself; 1e-4 of the reference
    for the FP32 exponentials and the sums).  -> (bC, bR, bT[, bD])."""
    nT = np.shape(pT)[1]
    d, b = _dvp4(dvp, nT, pD), _dvp4(bud, nT, pD)
    if pD is None:
        d, b, pD1 = d[..., None], b[..., None], np.ones((len(d), 1))
    else:
        pD1 = np.asarray(pD, np.float64)
    pC, pR, pT = (np.asarray(a, np.float64) for a in (pC, pR, pT))
    base = d.max(axis=(1, 2, 3))
    btop = b.max(axis=(1, 2, 3))
    m = np.exp(d - base[:, None, None, None]) * np.expm1(b + btop[:, None, None, None])
    ref = weights2d_64(dvp, pC, pR, pT, pD)
    bC = np.einsum("lrtd,lr,lt,ld->l", m, pR, pT, pD1)
    bR = pC[:, None] * np.einsum("lrtd,lt,ld->lr", m, pT, pD1)
    bT = pC[:, None] * np.einsum("lrtd,lr,ld->lt", m, pR, pD1)
    bD = pC[:, None] * np.einsum("lrtd,lr,lt->ld", m, pR, pT)
    bs = (bC, bR, bT, bD) if pD is not None else (bC, bR, bT)
    return tuple(x + 1e-4 * r for x, r in zip(bs, ref))


# ----------------------------------------------------------------- emulation
def emu_local2d_32(img, rot, trans, dat, ctf, sig, iCol, iRow, idim, pf, cls=None):
    """k_local2d's sums in FP32, operation by operation in its order: the FP64
    rotation rounded to FP32, interp2, phase_shift's FP32 argument (sin / cos
    of it taken in float64 and rounded), cmul, er, ei, (er er + ei ei) s, each
    thread's terms i = tid, tid + 256, ... in turn, the butterfly of wave_sum,
    the four waves in turn.  No contraction.  -> [nImg, nR, nT nD] float32."""
    f = np.float32
    rot = np.asarray(rot, np.float64)
    nImg = rot.shape[0]
    imgs = _per_image(img, cls, nImg)
    c3, _ = _ctf3(ctf)
    c3 = c3.astype(f)
    ic, ir = np.asarray(iCol, np.int64), np.asarray(iRow, np.int64)
    t32 = np.asarray(trans, np.float64).astype(f) / f(idim)               # [l, t, 2]
    rev = -(ic.astype(f) * t32[..., :1] + ir.astype(f) * t32[..., 1:])    # [l, t, i] FP32
    fr = (rev - np.rint(rev)).astype(np.float64)
    Tx, Ty = np.cos(2 * np.pi * fr).astype(f), np.sin(2 * np.pi * fr).astype(f)
    d, s = np.asarray(dat), np.asarray(sig, f)
    dr, di = d.real.astype(f), d.imag.astype(f)
    nR, nT, nD, nPxl = rot.shape[1], t32.shape[1], c3.shape[1], len(ic)
    pad = -(-nPxl // THREADS) * THREADS
    out = np.empty((nImg, nR, nT, nD), f)
    for l in range(nImg):
        P = emu_project2d_32(imgs[l], rot[l], iCol, iRow, pf)             # [r, i]
        pr, pi = P.real.astype(f)[:, None, :], P.imag.astype(f)[:, None, :]
        px = Tx[l][None] * pr - Ty[l][None] * pi                          # [r, t, i]
        py = Tx[l][None] * pi + Ty[l][None] * pr
        for k in range(nD):
            er = dr[l] - c3[l, k] * px
            ei = di[l] - c3[l, k] * py
            term = (er * er + ei * ei) * s[l]
            tp = np.zeros((nR, nT, pad), f)
            tp[..., :nPxl] = term
            tp = tp.reshape(nR, nT, pad // THREADS, THREADS)
            acc = np.zeros((nR, nT, THREADS), f)
            for j in range(tp.shape[2]):
                acc = acc + tp[:, :, j]
            v = acc.reshape(nR, nT, 4, 64)
            lanes = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                v = v + v[..., lanes ^ o]
            tot = np.zeros((nR, nT), f)
            for w in range(4):
                tot = tot + v[:, :, w, 0]
            out[l, :, :, k] = tot
    return out.reshape(nImg, nR, nT * nD)


# -------------------------------------------------------------------- insert
class Scatter2(SC.Scatter):
    """scatter_ref.Scatter over nK class maps (flat), with O [nK, 2], its
    magnitude sums and the per-class counters."""

    def __init__(self, size, nK):
        super().__init__(size * nK)
        self.O = np.zeros((nK, 2))
        self.aO = np.zeros((nK, 2))
        self.cnt = np.zeros(nK, np.int64)

    def bO(self):
        return (self.cnt[:, None] + 3) * 2.0 ** -53 * self.aO


def insert2d_64(vdim, pf, dat, ctf, rot, trans, off, w, nc, iCol, iRow, idim, nK=1, attr=None,
                nD=None, mut=None, round32=True):
    """The float64 insert of dat [nImg, nPxl] under rot / trans [nImg, mReco, 2],
    off [nImg, 2], w [nImg], nc [nImg, mReco] or None (class 0); ctf
    [nImg, nPxl], or attr [nImg, 8] with nD [nImg, mReco] (ctf = None).  mut:
    "noconj", "foldgt", "osign", "tctf", "clsfirst".  round32 = False keeps the
    FP64 coordinate (the exact adjoint of project2d_64)."""
    rot, trans, off = (np.asarray(a, np.float64) for a in (rot, trans, off))
    nImg, mReco = rot.shape[:2]
    iCol, iRow = np.asarray(iCol), np.asarray(iRow)
    ncol = vdim // 2 + 1
    size = ncol * vdim
    out = Scatter2(size, nK)
    for l in range(nImg):
        x, y = coords2_64(rot[l], iCol, iRow, pf)                                  # [m, i]
        if round32:
            x, y = x.astype(np.float32), y.astype(np.float32)
        conj = ~(x > 0) if mut == "foldgt" else ~(x >= 0)
        sg = np.where(conj, -1, 1).astype(x.dtype)
        xs, ys = x * sg, y * sg
        fx, fy = np.floor(xs), np.floor(ys)
        dx_, dy_ = xs.astype(np.float64) - fx, ys.astype(np.float64) - fy           # exact
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        assert x0.min() >= 0 and x0.max() + 1 < ncol, "tap outside the half-complex row"
        assert y0.min() >= -(vdim // 2) and y0.max() + 1 <= vdim // 2, "row outside the box"
        tx = (trans[l, :, 0] - off[l, 0])[:, None]
        ty = (trans[l, :, 1] - off[l, 1])[:, None]
        phase = np.exp(2j * np.pi * (iCol[None, :] * tx + iRow[None, :] * ty) / idim)
        theta = 2 * np.pi * (np.abs(iCol[None, :] * tx) + np.abs(iRow[None, :] * ty)) / idim
        wl = float(np.float32(w[l]))
        d = np.asarray(dat[l], np.complex64).astype(np.complex128)[None, :]
        if attr is None:
            c, dc = np.asarray(ctf[l], np.float32).astype(np.float64)[None, :], 0.0
        else:
            c, dc = SC.ctf_f64(attr[l], np.asarray(nD, np.float64)[l], iCol, iRow, idim)
        val = d * phase * c * wl
        if mut != "noconj":
            val = np.where(conj, np.conj(val), val)
        tv = (c if mut == "tctf" else c * c) * wl + np.zeros_like(theta)
        av = np.abs(val)
        eF = np.abs(d) * wl * dc / U + np.zeros_like(theta)
        eT = (2 * np.abs(c) + dc) * dc * wl / U + np.zeros_like(theta)
        if nc is None:
            k = np.zeros(mReco, np.int64)
        else:
            k = np.asarray(nc, np.int64)[l]
            k = np.full(mReco, k[0]) if mut == "clsfirst" else k
        for j in range(2):
            for i in range(2):
                yy = y0 + j
                yy = np.where(yy >= 0, yy, yy + vdim)
                idx = k[:, None] * size + yy * ncol + x0 + i
                wt = (dx_ if i else 1 - dx_) * (dy_ if j else 1 - dy_)
                np.add.at(out.F, idx, val * wt)
                np.add.at(out.T, idx, tv * wt)
                np.add.at(out.n, idx, 1)
                np.add.at(out.aF, idx, av * (2 + 10 * wt) + eF * wt)
                np.add.at(out.pF, idx, av * wt * 4 * theta)
                np.add.at(out.sF, idx, av * wt)
                np.add.at(out.aT, idx, np.abs(tv) * (2 + 10 * wt) + eT * wt)
                np.add.at(out.sT, idx, np.abs(tv) * wt)
        cs, sn = rot[l, :, 0], rot[l, :, 1]
        sgn = 1.0 if mut == "osign" else -1.0
        o = sgn * np.stack([cs * tx[:, 0] - sn * ty[:, 0], sn * tx[:, 0] + cs * ty[:, 0]], 1)
        ao = np.stack([np.abs(cs * tx[:, 0]) + np.abs(sn * ty[:, 0]),
                       np.abs(sn * tx[:, 0]) + np.abs(cs * ty[:, 0])], 1)
        np.add.at(out.O, k, o)
        np.add.at(out.aO, k, ao)
        np.add.at(out.cnt, k, 1)
    return out


def check_insert2d(gF, gT, gO, gcnt, ref, P):
    """The per-voxel check of an insert's F (complex, flat over the classes), T,
    O [nK, 2] and counters against ref (a Scatter2): scatter_ref.check_insert
    (every voxel within budget, exactly 0 outside the support), O within bO,
    the counters exact.  -> largest err / budget of (F.re, F.im, T, O)."""
    assert np.array_equal(np.asarray(gcnt, np.int64).reshape(-1), ref.cnt), "counters differ"
    r = SC.check_insert(np.asarray(gF).reshape(-1), np.asarray(gT).reshape(-1), ref, P)
    ro = worst(np.asarray(gO, np.float64).reshape(ref.O.shape), ref.O, ref.bO())
    assert ro <= 1, f"largest O err / bound {ro}"
    return r + (ro,)


def scaled(ref, times):
    """The reference of `times` identical inserts accumulated onto one map:
    the sums and n_v multiplied (the taps of a voxel are then times n_v)."""
    import copy
    r = copy.copy(ref)
    for k in ("F", "T", "n", "aF", "pF", "sF", "aT", "sT", "O", "aO", "cnt"):
        setattr(r, k, getattr(ref, k) * times)
    return r
