"""Seeded small edge cases of the 3D local phase, shared by the CPU check of
the reference (test_phase_ref.py) and the device check
(test_gpu_phase_edges.py).  Pure numpy.

Inputs of a case (exactly what thx_local_phase* gets):
  vol    the FFT of a real seeded blob volume (box N = 16 or 32 padded to
         vdim = 2 N), so its x = 0 plane is Hermitian; times the radial
         fall-off 1 / (1 + k / 8), scaled to a median magnitude of 1, and a DC
         voxel of 1000: no real pixel's taps reach it (a pixel's coordinate
         vector is at least pf = 2 long), but every padding entry of the cell
         layout samples pixel (0, 0);
  pixels the n lattice points nearest the origin with iCol >= 0, the origin
         left out, or the whole half-disc iCol^2 + iRow^2 < rU^2;
  quat   uniform, or clouds of the stated width about one centre per image;
         a rotation is redrawn until no sample of it has 0 < |x| < 1e-4 or a
         coordinate within 1e-4 of an integer it is not exactly equal to;
  ctf    sin(0.35 rho^2 + phase_l): in [-1, 1], with sign changes (ctfD: the
         same at defocus factors 1 + 0.05 d);
  sig    -10^U(-1, 1) per pixel (sigRcp = -1 / (2 sigma^2)), scaled per image
         so that sum |s| |d|^2 = 6: every dvp of an image then lies within a
         few tens of its maximum and no reference marginal underflows
         (`underflow`: 400);
  dat    c T P of a chosen pose of the cloud plus complex normal noise at the
         stated SNR;
  pC, pR, pT[, pD]  log-uniform over three decades, normalised (pC: 1).
"""
import numpy as np

import phase_ref as R

PF = 2
A_TARGET = 6.0


# -------------------------------------------------------------------- pieces
def volume(N, seed):
    vdim = PF * N
    rng = np.random.default_rng(seed)
    g = np.arange(vdim)
    g = np.where(g < vdim // 2, g, g - vdim).astype(np.float64)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    rho = np.zeros((vdim,) * 3)
    for _ in range(48):
        c = rng.uniform(-N / 3, N / 3, 3)
        rho += rng.uniform(0.3, 1.0) * np.exp(-((Z - c[0]) ** 2 + (Y - c[1]) ** 2 + (X - c[2]) ** 2) / (2 * 0.7 ** 2))
    F = np.fft.rfftn(rho)                                   # [z, y, x], x the half axis
    k = np.sqrt(Z ** 2 + Y ** 2 + X ** 2)[:, :, :vdim // 2 + 1]
    F = F / (1 + k / 8)
    F /= np.median(np.abs(F))
    F[0, 0, 0] = 1000.0
    return F.astype(np.complex64)


def pixels_nearest(n):
    r = int(np.ceil(np.sqrt(n))) + 2
    pts = [(x, y) for x in range(0, r + 1) for y in range(-r, r + 1) if (x, y) != (0, 0)]
    pts.sort(key=lambda p: (p[0] ** 2 + p[1] ** 2, p))
    p = np.array(pts[:n], np.int32)
    return p[:, 0].copy(), p[:, 1].copy()


def pixels_disc(rU):
    r = int(np.ceil(rU))
    pts = [(x, y) for x in range(0, r + 1) for y in range(-r, r + 1)
           if (x, y) != (0, 0) and x * x + y * y < rU * rU]
    pts.sort(key=lambda p: (p[0] ** 2 + p[1] ** 2, p))
    p = np.array(pts, np.int32)
    return p[:, 0].copy(), p[:, 1].copy()


def qmul(a, b):
    a0, a1, a2, a3 = (a[..., k] for k in range(4))
    b0, b1, b2, b3 = (b[..., k] for k in range(4))
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], -1)


def q_uniform(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def q_small(rng, n, deg):
    """Rotations by N(0, deg) degrees about uniform axes."""
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    h = np.deg2rad(rng.standard_normal(n) * deg) / 2
    return np.concatenate([np.cos(h)[:, None], np.sin(h)[:, None] * ax], 1)


def coords_ok(q, iCol, iRow):
    """Per rotation: the fold and the floor are decided alike in FP32 and FP64."""
    x, y, z = R.coords64(q, iCol, iRow, PF)
    ok = ~((np.abs(x) > 0) & (np.abs(x) < 1e-4)).any(-1)
    for a in (x, y, z):
        n = np.rint(a)
        ok &= ~((np.abs(a - n) < 1e-4) & (a != n)).any(-1)
    return ok


def clean(q, draw, iCol, iRow):
    """q [n, 4] with the rotations that fail coords_ok redrawn by draw(idx)."""
    for _ in range(100):
        bad = np.flatnonzero(~coords_ok(q, iCol, iRow))
        if not len(bad):
            return q
        q[bad] = draw(bad)
    raise AssertionError("no clean rotation found")


def log_uniform(rng, *shape):
    p = 10.0 ** rng.uniform(-3, 0, shape)
    return p / p.sum(-1, keepdims=True)


# ---------------------------------------------------------------------- make
def make(nImg, nR, nT, pix, seed, N=16, snr=0.5, cloud=None, nD=0, nK=1, a_target=A_TARGET,
         fixed=None, tr_range=3.0):
    """pix: (iCol, iRow).  cloud: None = uniform rotations, else the width in
    degrees of a cloud about one uniform centre per image.  fixed: [m, 4]
    rotations every image's list starts with (kept as given)."""
    rng = np.random.default_rng(seed)
    iCol, iRow = pix
    nPxl = len(iCol)
    vol = volume(N, seed) if nK == 1 else np.stack([volume(N, seed + 7 * k) for k in range(nK)])
    quat = np.empty((nImg, nR, 4))
    for l in range(nImg):
        if cloud is None:
            draw = lambda idx: q_uniform(rng, len(idx))
        else:
            ctr = q_uniform(rng, 1)
            draw = lambda idx, ctr=ctr: qmul(ctr, q_small(rng, len(idx), cloud))
        nF = 0 if fixed is None else len(fixed)
        if nF:
            quat[l, :nF] = fixed
        quat[l, nF:] = clean(draw(np.arange(nR - nF)), draw, iCol, iRow)
    trans = rng.uniform(-tr_range, tr_range, (nImg, nT, 2))
    rho = np.hypot(iCol, iRow)
    ph = rng.uniform(0, 2 * np.pi, (nImg, 1))
    ctf = np.sin(0.35 * rho[None, :] ** 2 + ph).astype(np.float32)
    cls = rng.integers(0, nK, nImg).astype(np.int32) if nK > 1 else None
    if cls is not None:
        cls[:2] = (0, 1)
    ir, it = rng.integers(0, nR, nImg), rng.integers(0, nT, nImg)
    c = dict(vol=vol, quat=quat, trans=trans, iCol=iCol, iRow=iRow, idim=N, pf=PF, vdim=PF * N,
             cls=cls, nD=nD, dims=(nImg, nR, nT, nPxl), pose=(ir, it), route=None,
             pC=np.ones(nImg), pR=log_uniform(rng, nImg, nR), pT=log_uniform(rng, nImg, nT))
    if nD:
        ctfD = np.stack([np.sin(0.35 * (1 + 0.05 * d) * rho[None, :] ** 2 + ph) for d in range(nD)], 1)
        c["ctfD"] = ctfD.astype(np.float32)
        c["pD"] = log_uniform(rng, nImg, nD)
        ctf = c["ctfD"][:, rng.integers(nD)]
    P = R.project64(vol, quat, iCol, iRow, PF, cls)
    T, _ = R.phases(trans, iCol, iRow, N)
    sigl = ctf * T[np.arange(nImg), it] * P[np.arange(nImg), ir]
    npow = np.maximum((np.abs(sigl) ** 2).mean(1, keepdims=True), 1e-3) / snr
    noise = (rng.standard_normal((nImg, nPxl)) + 1j * rng.standard_normal((nImg, nPxl))) * np.sqrt(npow / 2)
    dat = (sigl + noise).astype(np.complex64)
    s = 10.0 ** rng.uniform(-1, 1, (nImg, nPxl))
    s *= a_target / (s * np.abs(dat) ** 2).sum(1, keepdims=True)
    c.update(dat=dat, ctf=ctf, sig=(-s).astype(np.float32), P=P)
    return c


PIX = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)
ROT = (1, 15, 16, 17, 127, 128, 129, 257)
TR = (1, 15, 16, 17, 33, 63, 64, 65)
TR_NR = (3, 129)
CS = {16: (16, 1), 17: (17, 1), 32: (32, 1), 33: (11, 3), 64: (64, 1), 65: (13, 5), 96: (32, 3),
      97: (97, 1), 1024: (64, 16)}            # columns: (nT, nD); 97 is prime, 1024 = LOCAL_D_MAXCOL
FOLD_FIXED = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]], np.float64)


def build(cid):
    name, _, arg = cid.partition("-")
    p17 = pixels_nearest(17)
    if cid == "one":
        return make(1, 1, 1, pixels_nearest(1), 1)
    if name == "pix":
        return make(3, 9, 5, pixels_nearest(int(arg)), 100 + int(arg))
    if cid == "rot-dup":
        # one tile of 128 copies of a rotation, q and -q in turn, then two others
        c = make(2, 130, 5, p17, 290)
        for l in range(2):
            c["quat"][l, :128] = c["quat"][l, 128]
            c["quat"][l, 1:128:2] *= -1
        return remake(c, 291)
    if name == "rot":
        return make(3, int(arg), 5, p17, 200 + int(arg))
    if name == "tr":
        nT, nR = (int(a) for a in arg.split("x"))
        return make(2, nR, nT, p17, 300 + nT + nR)
    if cid == "fold":
        # identity and the three half turns: every coordinate an integer, x = +-0
        # on the iCol = 0 pixels; then a 2 degree cloud about the identity, whose
        # iCol = 0 pixels land on both sides of x = 0 inside the first cell
        c = make(2, 33, 5, pixels_disc(6), 400, fixed=FOLD_FIXED)
        rng = np.random.default_rng(401)
        for l in range(2):
            draw = lambda idx: q_small(rng, len(idx), 2.0)
            c["quat"][l, 4:] = clean(draw(np.arange(29)), draw, c["iCol"], c["iRow"])
        return remake(c, 402)
    if cid == "wrap":
        return make(2, 33, 5, pixels_disc(8), 500)
    if cid in ("narrow", "wide", "wide-129", "mixed", "ball-edge"):
        # the route's sample is image 0: under uniform rotations the patches of
        # a full tile of 128 do not fit the LDS box, those of a tile of one do.
        # nR 257 is two tiles against one (the box-less / y-pair kernel);
        # nR 129 one against one, which the 50 per cent threshold leaves to the
        # staged kernel: its first tile gathers every patch directly
        cloud = {"narrow": 1.0, "mixed": 8.0}.get(cid)
        nR = 257 if cid in ("wide", "ball-edge") else 129
        c = make(3, nR, 9, pixels_disc(12), 600 if cid == "ball-edge" else 601 + len(cid), N=32, cloud=cloud)
        c["route"] = {"narrow": (0, 0), "wide": (1, 2), "ball-edge": (1, 2), "wide-129": (0, 0)}.get(cid)
        return c
    if cid in ("nobox-rot", "nobox-tr"):
        # rot-257 and tr-17 on 33 pixels, whose patch boxes do not fit: the tile
        # edges of the box-less half-complex kernel and of the routed y-pair one
        c = make(3, 257, 5, pixels_nearest(33), 650) if cid == "nobox-rot" else \
            make(3, 9, 17, pixels_nearest(33), 651)
        c["route"] = (1, 2)
        return c
    if cid == "route-65":
        return make(65, 3, 3, p17, 700)
    if cid == "priors":
        c = make(3, 9, 5, p17, 800)
        c["pC"] = np.array([0.25, 3.0, 1e-2])
        for l in range(3):
            c["pR"][l, [l, 8 - l]] = 0.0
            c["pT"][l, [l % 5, (l + 2) % 5]] = 0.0
        return c
    if cid == "underflow":
        return make(3, 9, 5, p17, 900, snr=1e4, a_target=400.0)
    if cid == "ties":
        c = make(3, 9, 5, p17, 1000, snr=20.0)
        for l in range(3):
            r = c["pose"][0][l]
            c["quat"][l, (r + 1) % 9] = c["quat"][l, r]
        return c
    if name == "cs":
        nT, nD = CS[int(arg)]
        return make(3, 2 if arg == "1024" else 9, nT, p17, 1100 + int(arg), nD=nD)
    if cid == "classes":
        return make(5, 9, 5, p17, 1200, nK=2, snr=4.0)
    raise KeyError(cid)


def remake(c, seed):
    """The images of a case whose rotations were edited after make(): dat and
    sig again from the edited cloud."""
    nImg, nR, nT, nPxl = c["dims"]
    rng = np.random.default_rng(seed)
    ir, it = c["pose"]
    P = R.project64(c["vol"], c["quat"], c["iCol"], c["iRow"], PF, c["cls"])
    T, _ = R.phases(c["trans"], c["iCol"], c["iRow"], c["idim"])
    sigl = c["ctf"] * T[np.arange(nImg), it] * P[np.arange(nImg), ir]
    npow = np.maximum((np.abs(sigl) ** 2).mean(1, keepdims=True), 1e-3) / 0.5
    noise = (rng.standard_normal((nImg, nPxl)) + 1j * rng.standard_normal((nImg, nPxl))) * np.sqrt(npow / 2)
    dat = (sigl + noise).astype(np.complex64)
    s = 10.0 ** rng.uniform(-1, 1, (nImg, nPxl))
    s *= A_TARGET / (s * np.abs(dat) ** 2).sum(1, keepdims=True)
    c.update(dat=dat, sig=(-s).astype(np.float32), P=P)
    return c


PLAIN = (["one"] + [f"pix-{n}" for n in PIX] + [f"rot-{n}" for n in ROT] + ["rot-dup"] +
         [f"tr-{t}x{r}" for t in TR for r in TR_NR] +
         ["nobox-rot", "nobox-tr", "fold", "wrap", "narrow", "wide", "wide-129", "mixed", "ball-edge", "route-65", "priors", "underflow",
          "ties", "classes"])
SEARCH = [f"cs-{n}" for n in CS]
ALL = PLAIN + SEARCH

_cache = {}


def args(c, search=None):
    """The reference's argument list of a case (ctfD for a search case)."""
    search = bool(c["nD"]) if search is None else search
    return (c["vol"], c["quat"], c["trans"], c["dat"], c["ctfD"] if search else c["ctf"], c["sig"],
            c["iCol"], c["iRow"], c["idim"], c["pf"], c["cls"])


def get(cid):
    """(case, dvp64, budget) of a case, computed once."""
    if cid not in _cache:
        c = build(cid)
        if cid == "ties":
            c.pop("P")          # a rotation edited after make(): project again
        a = args(c)
        d64 = R.dvp64(*a, P=c.get("P"))
        _cache[cid] = (c, d64, R.budget(R.sums(*a), c["dims"][3]))
    return _cache[cid]
