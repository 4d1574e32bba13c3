"""Seeded small edge cases of the 2D classification kernels (csrc/twod.hip),
shared by the CPU check of the reference (test_twod_ref.py) and the device
check (test_gpu_twod_edges.py).  Pure numpy.

Inputs of a case (exactly what the entry points get):
  img    nK Hermitian class images: the rfft2 of real seeded blobs (sigma 0.7
         pixels, so every radius carries signal) on the padded box
         vdim = pf N, times the radial fall-off 1 / (1 + k / 8), scaled to a
         median magnitude of 1; the x = 0 column's symmetry
         F[-j, 0] = conj F[j, 0] is pinned exactly (and asserted), so the
         gather is continuous across the fold;
  pixels the n lattice points nearest the origin with iCol >= 0, the origin
         left out (phase_cases.pixels_nearest), a half-disc, or a hand-made
         list; N is the smallest multiple of 16 (>= 16) whose half N / 2
         exceeds the list's largest radius, so every tap of every rotation
         is in range;
  rot    (cos, sin) of uniform angles; a rotation is redrawn until
         twod_ref.fused_agree holds for it and no sample of it has
         0 < |x| < 1e-4 or a coordinate within 1e-4 of an integer it is not
         equal to; the on-grid rotations (1, 0), (0, 1), (-1, 0), (0, -1) have
         exact products and are kept as given;
  ctf    sin(0.9 rho^2 + phase_l): mixed sign (ctfD: the same at defocus
         factors 1 + 0.05 d);
  sig    -10^U(-1, 1) per pixel (sigRcp = -1 / (2 sigma^2)), scaled per image
         so that sum |s| |d|^2 = 6;
  dat    c T P of a chosen pose plus complex normal noise at SNR 0.5;
  pC, pR, pT[, pD]  log-uniform over three decades, normalised (pC
         non-uniform in [0.25, 3]).
"""
import numpy as np

import phase_cases as PC
import phase_ref as PR
import twod_ref as R

PF = 2
A_TARGET = 6.0
GRID = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])


# -------------------------------------------------------------------- pieces
def classes(nK, N, pf, seed):
    """[nK, vdim, vdim/2+1] complex64, Hermitian, the x = 0 column pinned."""
    vdim = N * pf
    rng = np.random.default_rng(seed)
    g = np.arange(vdim)
    g = np.where(g < vdim // 2, g, g - vdim).astype(np.float64)
    Y, X = np.meshgrid(g, g, indexing="ij")
    k = np.sqrt(Y ** 2 + X ** 2)[:, :vdim // 2 + 1]
    out = np.empty((nK, vdim, vdim // 2 + 1), np.complex64)
    for q in range(nK):
        rho = np.zeros((vdim, vdim))
        for _ in range(24):
            c = rng.uniform(-N / 3, N / 3, 2)
            rho += rng.uniform(0.3, 1.0) * np.exp(-((Y - c[0]) ** 2 + (X - c[1]) ** 2) / (2 * 0.7 ** 2))
        F = np.fft.rfft2(rho) / (1 + k / 8)
        F = (F / np.median(np.abs(F))).astype(np.complex64)
        j = np.arange(1, vdim // 2)
        F[vdim - j, 0] = np.conj(F[j, 0])
        F[0, 0] = F[0, 0].real
        F[vdim // 2, 0] = F[vdim // 2, 0].real
        out[q] = F
    assert hermitian_x0(out)
    return out


def hermitian_x0(img):
    img = np.asarray(img).reshape(-1, img.shape[-2], img.shape[-1])
    vdim = img.shape[1]
    j = np.arange(vdim)
    return bool((img[:, (-j) % vdim, 0] == np.conj(img[:, j, 0])).all())


def box_for(iCol, iRow):
    r = float(np.sqrt((np.asarray(iCol, np.int64) ** 2 + np.asarray(iRow, np.int64) ** 2).max()))
    N = 16
    while N / 2 <= r:
        N += 16
    return N


def rot_of(th):
    return np.stack([np.cos(th), np.sin(th)], -1)


def margin(iCol):
    """The distance a coordinate keeps from an integer it is not equal to:
    1e-4; 2e-5 for the lists of thousands of pixels, where 1e-4 leaves too few
    rotations (an FP32 coordinate below 128 is rounded by at most 4e-6)."""
    return 1e-4 if len(iCol) < 3000 else 2e-5


def rot_ok(rot, iCol, iRow, pf):
    """Per rotation: fused and unfused agree, and fold and floor are decided
    alike in FP32 and FP64."""
    x, y = R.coords2_64(rot, iCol, iRow, pf)
    mg = margin(iCol)
    ok = ~((np.abs(x) > 0) & (np.abs(x) < mg)).any(-1)
    for a in (x, y):
        n = np.rint(a)
        ok &= ~((np.abs(a - n) < mg) & (a != n)).any(-1)
    return ok & R.fused_agree(rot, iCol, iRow, pf)


def draw_rot(rng, n, iCol, iRow, pf):
    rot = rot_of(rng.uniform(0, 2 * np.pi, n))
    for _ in range(100):
        bad = np.flatnonzero(~rot_ok(rot, iCol, iRow, pf))
        if not len(bad):
            return rot
        rot[bad] = rot_of(rng.uniform(0, 2 * np.pi, len(bad)))
    raise AssertionError("no clean rotation found")


# ---------------------------------------------------------------------- make
def make(nImg, nR, nT, pix, seed, nD=0, nK=1, cls=None, fixed=None, N=None, pf=PF):
    """A local-phase case.  fixed: [m, 2] rotations every image's list starts
    with (kept as given)."""
    rng = np.random.default_rng(seed)
    iCol, iRow = (np.asarray(a, np.int32) for a in pix)
    nPxl = len(iCol)
    N = box_for(iCol, iRow) if N is None else N
    vdim = N * pf
    img = classes(nK, N, pf, seed)
    nF = 0 if fixed is None else len(fixed)
    rot = np.empty((nImg, nR, 2))
    for l in range(nImg):
        if nF:
            rot[l, :nF] = fixed
        if nR > nF:
            rot[l, nF:] = draw_rot(rng, nR - nF, iCol, iRow, pf)
    trans = rng.uniform(-3.0, 3.0, (nImg, nT, 2))
    rho = np.hypot(iCol, iRow)
    ph = rng.uniform(0, 2 * np.pi, (nImg, 1))
    ctf = np.sin(0.9 * rho[None, :] ** 2 + ph).astype(np.float32)
    if nK > 1 and cls is None:
        cls = np.arange(nImg)[::-1] % nK
    cls = None if cls is None else np.asarray(cls, np.int32)
    c = dict(img=img if nK > 1 else img[0], rot=rot, trans=trans, iCol=iCol, iRow=iRow, idim=N, pf=pf,
             vdim=vdim, cls=cls, nK=nK, nD=nD, dims=(nImg, nR, nT, nPxl),
             pC=rng.uniform(0.25, 3.0, nImg), pR=PC.log_uniform(rng, nImg, nR),
             pT=PC.log_uniform(rng, nImg, nT))
    if nD:
        ctfD = np.stack([np.sin(0.9 * (1 + 0.05 * d) * rho[None, :] ** 2 + ph) for d in range(nD)], 1)
        c["ctfD"] = ctfD.astype(np.float32)
        c["pD"] = PC.log_uniform(rng, nImg, nD)
        ctf = c["ctfD"][:, rng.integers(nD)]
    ir, it = rng.integers(0, nR, nImg), rng.integers(0, nT, nImg)
    P = R.project2d_64(c["img"], rot, iCol, iRow, pf, cls)
    T, _ = PR.phases(trans, iCol, iRow, N)
    sigl = ctf * T[np.arange(nImg), it] * P[np.arange(nImg), ir]
    npow = np.maximum((np.abs(sigl) ** 2).mean(1, keepdims=True), 1e-3) / 0.5
    noise = (rng.standard_normal((nImg, nPxl)) + 1j * rng.standard_normal((nImg, nPxl))) * np.sqrt(npow / 2)
    dat = (sigl + noise).astype(np.complex64)
    s = 10.0 ** rng.uniform(-1, 1, (nImg, nPxl))
    s *= A_TARGET / (s * np.abs(dat) ** 2).sum(1, keepdims=True)
    c.update(dat=dat, ctf=ctf, sig=(-s).astype(np.float32), P=P)
    return c


PIX = (1, 63, 64, 65, 255, 256, 257, 513)
COL = (1, 15, 16, 17, 32, 33)
CS = ((5, 3), (3, 7), (16, 2), (8, 4), (1, 17), (65, 3), (64, 16))     # (nT, nD); 64 x 16 = 1024
INS_PIX = (1, 255, 256, 257, 2048, 2049)


def ring(r0, r1):
    ic, ir = PC.pixels_disc(r1)
    m = ic.astype(np.int64) ** 2 + ir.astype(np.int64) ** 2 >= r0 * r0
    return ic[m], ir[m]


def grid_pixels():
    """A half-disc of radius < 7 (N 16, pf 2: coordinates below 14) with the
    iCol = 0 pixels of both row signs, the iRow = 0 pixels and the outermost
    ring in it."""
    ic, ir = PC.pixels_disc(7)
    assert ((ic == 0) & (ir < 0)).any() and ((ic == 0) & (ir > 0)).any() and (ir == 0).any()
    return ic, ir


def build(cid):
    name, _, arg = cid.partition("-")
    p17 = PC.pixels_nearest(17)
    if name == "pix":
        return make(2, 3, 3, PC.pixels_nearest(int(arg)), 100 + int(arg))
    if name == "col":
        return make(2, 2, int(arg), p17, 200 + int(arg))
    if name == "cs":
        nT, nD = (int(a) for a in arg.split("x"))
        if nT * nD == 1024:
            return make(1, 1, nT, PC.pixels_nearest(16), 300, nD=nD)
        return make(2, 2, nT, p17, 300 + nT + nD, nD=nD)
    if cid == "rot-1":
        return make(2, 1, 3, p17, 400)
    if cid == "rot-dup":
        c = make(2, 3, 3, p17, 401)
        return make(2, 3, 3, p17, 401, fixed=c["rot"][0, 2:3].repeat(2, 0))
    if cid == "fold-grid":
        return make(2, 8, 3, grid_pixels(), 500, fixed=GRID)
    if cid == "edge-ring":
        # N 16, pf 2: pixel (7, 3) at radius 7.62 lands on x in [15, 16) and on
        # y in [15, 16) and [-16, -15) under the three fixed rotations
        a = np.arctan2(3.0, 7.0)
        fixed = rot_of(np.array([-a + 0.02, np.pi / 2 - a - 0.02, -np.pi / 2 - a + 0.02]))
        return make(2, 6, 3, PC.pixels_disc(8), 600, fixed=fixed)
    if cid in ("lds-190", "global-192", "lds-190-k", "global-192-k"):
        N = 95 if cid.startswith("lds") else 96
        k = cid.endswith("-k")
        return make(2, 3, 3, ring(6, 14), 700 + N + k, N=N, nK=3 if k else 1, cls=[2, 1] if k else None)
    if cid == "cls-null":
        return make(1, 3, 3, p17, 800)
    if cid == "cls-k":
        return make(4, 3, 3, p17, 801, nK=3, cls=[2, 0, 1, 2])
    raise KeyError(cid)


PLAIN = ([f"pix-{n}" for n in PIX] + [f"col-{n}" for n in COL] +
         ["rot-1", "rot-dup", "fold-grid", "edge-ring", "lds-190", "global-192", "lds-190-k", "global-192-k",
          "cls-null", "cls-k"])
SEARCH = [f"cs-{t}x{d}" for t, d in CS]
LOCAL = PLAIN + SEARCH

_cache = {}


def args(c):
    return (c["img"], c["rot"], c["trans"], c["dat"], c["ctfD"] if c["nD"] else c["ctf"], c["sig"],
            c["iCol"], c["iRow"], c["idim"], c["pf"], c["cls"])


def get(cid):
    """(case, dvp2d_64, budget) of a local-phase case, computed once."""
    if cid not in _cache:
        c = build(cid)
        a = args(c)
        _cache[cid] = (c, R.dvp2d_64(*a, P=c["P"]), R.dvp_budget(R.sums2d(*a), c["dims"][3]))
    return _cache[cid]


# ---------------------------------------------------------------- projection
def proj_cases():
    return ["proj-cap", "fold-grid", "edge-ring", "pix-257"]


def get_proj(cid):
    """(img [vdim, nc], rot [nR, 2], iCol, iRow, pf, vdim) of a projection case."""
    key = ("proj", cid)
    if key not in _cache:
        if cid == "proj-cap":
            iCol, iRow = PC.pixels_nearest(8193)
            N, pf = 160, 1
            assert box_for(iCol, iRow) <= N
            rng = np.random.default_rng(900)
            _cache[key] = (classes(1, N, pf, 900)[0], draw_rot(rng, 2, iCol, iRow, pf), iCol, iRow, pf, N * pf)
        else:
            c, _, _ = get(cid)
            _cache[key] = (c["img"], c["rot"][0], c["iCol"], c["iRow"], c["pf"], c["vdim"])
    return _cache[key]


# -------------------------------------------------------------------- insert
def make_insert(nImg, mReco, pix, seed, nK=1, nc=None, fixed=None, search=False):
    rng = np.random.default_rng(seed)
    iCol, iRow = (np.asarray(a, np.int32) for a in pix)
    nPxl = len(iCol)
    N = box_for(iCol, iRow)
    nF = 0 if fixed is None else len(fixed)
    rot = np.empty((nImg, mReco, 2))
    for l in range(nImg):
        if nF:
            rot[l, :nF] = fixed
        if mReco > nF:
            rot[l, nF:] = draw_rot(rng, mReco - nF, iCol, iRow, PF)
    dat = (rng.standard_normal((nImg, nPxl)) + 1j * rng.standard_normal((nImg, nPxl))).astype(np.complex64)
    rho = np.hypot(iCol, iRow)
    ctf = np.sin(0.9 * rho[None, :] ** 2 + rng.uniform(0, 2 * np.pi, (nImg, 1))).astype(np.float32)
    c = dict(rot=rot, quat=rot, trans=rng.uniform(-3, 3, (nImg, mReco, 2)), off=rng.standard_normal((nImg, 2)) * 0.2,
             w=rng.uniform(0.1, 0.3, nImg).astype(np.float32), dat=dat, ctf=ctf, iCol=iCol, iRow=iRow,
             idim=N, pf=PF, vdim=N * PF, nK=nK, nc=None if nc is None else np.asarray(nc, np.int32),
             attr=None, nD=None, dims=(nImg, mReco, nPxl))
    if search:
        import insert_cases
        c["attr"], c["nD"] = insert_cases.ctf_search_inputs(c, seed)
    return c


def build_insert(cid):
    if cid.startswith("ins-pix-"):
        n = int(cid.rsplit("-", 1)[1])
        return make_insert(2, 2, PC.pixels_nearest(n), 1000 + n)
    if cid == "ins-grid":
        return make_insert(2, 8, grid_pixels(), 1100, fixed=GRID)
    if cid == "ins-cls":
        # nK 4: class 2 never drawn, the last class drawn, every image's first
        # sample of another class than its later ones
        return make_insert(3, 4, PC.pixels_nearest(65), 1200, nK=4,
                           nc=[[0, 3, 1, 3], [3, 0, 0, 1], [1, 1, 3, 0]])
    if cid == "ins-cls1":
        return make_insert(2, 3, PC.pixels_nearest(65), 1201)
    if cid == "ins-d":
        return make_insert(2, 2, PC.pixels_nearest(257), 1300, search=True)
    if cid == "ins-d-cls":
        return make_insert(2, 3, PC.pixels_nearest(65), 1301, nK=3, nc=[[2, 0, 2], [1, 2, 0]], search=True)
    raise KeyError(cid)


INSERT = [f"ins-pix-{n}" for n in INS_PIX] + ["ins-grid", "ins-cls", "ins-cls1", "ins-d", "ins-d-cls"]


def insert_args(c):
    return (c["vdim"], c["pf"], c["dat"], None if c["attr"] is not None else c["ctf"], c["rot"], c["trans"],
            c["off"], c["w"], c["nc"], c["iCol"], c["iRow"], c["idim"])


def get_insert(cid):
    """(case, insert2d_64) of an insert case, computed once."""
    key = ("ins", cid)
    if key not in _cache:
        c = build_insert(cid)
        _cache[key] = (c, R.insert2d_64(*insert_args(c), nK=c["nK"], attr=c["attr"], nD=c["nD"]))
    return _cache[key]


# --------------------------------------------------------------- global scan
G2D = {"g2d-1-1-1": (1, 1, 1), "g2d-69-24-9": (69, 24, 9), "g2d-69-1-9": (69, 1, 9), "g2d-1-24-1": (1, 24, 1)}
G2D_NK, G2D_NIMG = 3, 3


def get_g2d(cid):
    """A thx_ExpectGlobal2D case: nK 3 classes, 3 images, shared rot [nR, 2],
    trans [nT, 2], pR [nR], pT [nT]; built once."""
    key = ("g2d", cid)
    if key not in _cache:
        nPxl, nR, nT = G2D[cid]
        seed = 1400 + nPxl + nR + nT
        c = make(G2D_NIMG, nR, nT, PC.pixels_nearest(nPxl), seed, nK=G2D_NK, cls=[0, 1, 2])
        c["rot"] = np.ascontiguousarray(c["rot"][0])
        c["trans"] = np.ascontiguousarray(c["trans"][0])
        c["pR"], c["pT"] = c["pR"][0].copy(), c["pT"][0].copy()
        _cache[key] = c
    return _cache[key]
