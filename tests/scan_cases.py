"""Seeded synthetic edge cases of the global scan, shared by the CPU check of
the reference (test_scan_ref.py) and the device check (test_gpu_scan_edges.py).

Inputs of a case (numpy, exactly what the kernels get):
  traP  exp(-2 pi i (x dx + y dy) / N) on an integer pixel list, rounded to
        complex64 (N = 64; the nPxl lattice points nearest the origin with
        x >= 0, the origin left out);
  rotP  complex normal times the radial fall-off 1 / (1 + rho / 4);
  ctf   sin(0.35 rho^2 + phase_l): in [-1, 1], with sign changes;
  sig   sign * 10^U(-1, 1) per pixel: two decades, then scaled per image so
        that sum |s| |d|^2 = 6 -- the scale of sigRcp is free (the guard's
        ratio does not see it), and this one keeps every dvp of an image
        within a few tens of its maximum, so no reference marginal
        underflows.  sign = +1 unless the case says -1, the sign of the
        product's sigRcp = -1 / (2 sigma^2);
  dat   ctf T P of a chosen grid pose plus complex normal noise at the
        stated SNR (signal power / noise power per image);
  pR, pT  log-uniform over three decades, normalised.
"""
import numpy as np

N = 64
A_TARGET = 6.0


def pixels(nPxl):
    r = int(np.ceil(np.sqrt(nPxl))) + 2
    pts = [(x, y) for x in range(0, r + 1) for y in range(-r, r + 1) if (x, y) != (0, 0)]
    pts.sort(key=lambda p: (p[0] ** 2 + p[1] ** 2, p))
    return np.array(pts[:nPxl], np.float64)


def log_uniform(rng, n):
    p = 10.0 ** rng.uniform(-3, 0, n)
    return p / p.sum()


def make(nImg, nR, nT, nPxl, seed, snr=0.5, sign=1.0, same_pose=False, nK=1, pose_r=None, tr_range=5.0,
         rot_spread=None):
    rng = np.random.default_rng(seed)
    px = pixels(nPxl)
    rho = np.hypot(px[:, 0], px[:, 1])
    tr = rng.uniform(-tr_range, tr_range, (nT, 2))
    traP = np.exp(-2j * np.pi * (tr[:, :1] * px[None, :, 0] + tr[:, 1:] * px[None, :, 1]) / N).astype(np.complex64)
    rot = [((rng.standard_normal((nR, nPxl)) + 1j * rng.standard_normal((nR, nPxl))) / (1 + rho / 4))
           .astype(np.complex64) for _ in range(nK)]
    if rot_spread is not None:      # every rotation within rot_spread of rotation 0
        rot = [(r[:1] + np.float32(rot_spread) * r).astype(np.complex64) for r in rot]
    ctf = np.sin(0.35 * rho[None, :] ** 2 + rng.uniform(0, 2 * np.pi, (nImg, 1))).astype(np.float32)
    ir = np.full(nImg, rng.integers(nR)) if same_pose else rng.integers(0, nR, nImg)
    it = np.full(nImg, rng.integers(nT)) if same_pose else rng.integers(0, nT, nImg)
    if pose_r is not None:
        ir = np.array(pose_r)
    sigl = ctf.astype(np.float64) * traP[it].astype(np.complex128) * rot[0][ir].astype(np.complex128)
    npow = np.maximum((np.abs(sigl) ** 2).mean(1, keepdims=True), 1e-3) / snr
    noise = (rng.standard_normal((nImg, nPxl)) + 1j * rng.standard_normal((nImg, nPxl))) * np.sqrt(npow / 2)
    dat = (sigl + noise).astype(np.complex64)
    s = 10.0 ** rng.uniform(-1, 1, (nImg, nPxl))
    s *= A_TARGET / (s * np.abs(dat) ** 2).sum(1, keepdims=True)
    c = dict(rotP=rot[0], rotK=rot, traP=traP, dat=dat, ctf=ctf, sig=(sign * s).astype(np.float32),
             pR=log_uniform(rng, nR), pT=log_uniform(rng, nT), pose=(ir, it), nK=nK, guard=None,
             dims=(nImg, nR, nT, nPxl))
    return c


def one():
    return make(1, 1, 1, 1, 1)


def chunks(nPxl):
    """nCk 1, 1, 2, 3 at nPxl 15, 16, 17, 33."""
    return make(3, 9, 5, nPxl, 100 + nPxl)


def img_tiles(nImg):
    """nIT 1, 1, 2, 3 at nImg 63, 64, 65, 129; nR 17: 3 rotation blocks of the split scan."""
    return make(nImg, 17, 5, 17, 200 + nImg)


def rot_edges(nR):
    return make(3, nR, 5, 17, 300 + nR)


ROT_BLOCKS_POSE = (2050, 2056)


def rot_blocks():
    """nRB 258 (split) and 515 (algo 1).  sign -1 and SNR 4 at rotations 2050
    and 2056, so each image's maximum sits in a rotation block that only a
    later stride trip of the combine kernels reads (256 and 257 of the split
    scan, 512 and 514 of algo 1)."""
    return make(2, 2057, 3, 17, 400, snr=4.0, sign=-1.0, pose_r=ROT_BLOCKS_POSE)


def frag_edges(nT):
    return make(3, 9, nT, 17, 500 + nT)


def pad_max(nT):
    """Every real sample has a negative cross term X, so a padded translation
    column (X = 0, dvp = A + B) would be the largest of its row: all
    rotations within 5 % of one projection, shifts under 0.05 px, the images
    that projection at SNR 20."""
    return make(3, 9, nT, 17, 1500 + nT, snr=20.0, tr_range=0.05, rot_spread=0.05)


def wide(nT):
    return make(3, 5, nT, 17, 600 + nT)


def priors():
    """pR and pT over three decades, each with two exact zeros, one at index 0."""
    c = make(5, 19, 37, 33, 700, sign=-1.0)
    for p, j in ((c["pR"], 11), (c["pT"], 20)):
        p[0] = p[j] = 0.0
        p /= p.sum()
    return c


MERGE_SCALE = (1.0, 1.6, 0.4)     # sign +1: a larger P raises the largest dvp: mid, high, low


def merge():
    """Three classes whose maxima are ordered mid, high, low."""
    c = make(5, 9, 5, 17, 800, nK=3)
    c["rotK"] = [(r * np.float32(k)).astype(np.complex64) for r, k in zip(c["rotK"], MERGE_SCALE)]
    c["rotP"] = c["rotK"][0]
    return c


def guard_all():
    c = make(65, 9, 33, 17, 900, snr=1.0, sign=-1.0)
    c["guard"] = 0.5
    return c


def guard_rounds():
    """All 64 images at one grid pose (r*, t*) at SNR 20: the wave that owns
    r* flags more than GCAP = 32 samples."""
    c = make(64, 9, 33, 33, 1000, snr=20.0, sign=-1.0, same_pose=True)
    c["guard"] = 4.0
    return c


def sparse():
    """Image 0 all zero, image 1 with ctf all zero, image 2 with sigRcp zero
    on half its pixels."""
    c = make(4, 9, 5, 17, 1100)
    c["dat"][0] = 0
    c["ctf"][1] = 0
    c["sig"][2, ::2] = 0
    return c


UNDERFLOW_R, UNDERFLOW_SCALE = 4, 14.0


def underflow():
    """Rotation 4's rotP scaled so that its samples sit more than 200 below
    the maximum (sign -1)."""
    c = make(2, 9, 5, 17, 1200, sign=-1.0)
    c["rotP"][UNDERFLOW_R] *= np.float32(UNDERFLOW_SCALE)
    return c


NAN_IMG = 3


def nan_image():
    """(with, without): image 3 holds one NaN pixel / that pixel set to 0."""
    c = make(65, 9, 5, 17, 1300)
    z = dict(c, dat=c["dat"].copy())
    z["dat"][NAN_IMG, 5] = 0
    c["dat"][NAN_IMG, 5] = complex(np.nan, 0.0)
    return c, z


CHUNKS = (15, 16, 17, 33)
IMG_TILES = (63, 64, 65, 129)
ROT_EDGES = (1, 7, 8, 9, 63, 64, 65)
FRAG_EDGES = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160)
FRAG_EDGES_DIRECT = (15, 16, 17)       # algo 0's 16-translation chunks
PAD_MAX = (1, 31, 33, 65, 97, 129)
WIDE = (161, 192, 193, 224, 225, 256)


def plain_cases():
    """(id, builder) of every single-class case compared sample by sample."""
    out = [("one", one)]
    out += [(f"chunks-{n}", lambda n=n: chunks(n)) for n in CHUNKS]
    out += [(f"img_tiles-{n}", lambda n=n: img_tiles(n)) for n in IMG_TILES]
    out += [(f"rot_edges-{n}", lambda n=n: rot_edges(n)) for n in ROT_EDGES]
    out += [("rot_blocks", rot_blocks)]
    out += [(f"frag_edges-{n}", lambda n=n: frag_edges(n)) for n in FRAG_EDGES]
    out += [(f"pad_max-{n}", lambda n=n: pad_max(n)) for n in PAD_MAX]
    out += [("priors", priors), ("guard_all", guard_all), ("guard_rounds", guard_rounds),
            ("sparse", sparse), ("underflow", underflow)]
    return out


_cache = {}


def get(cid):
    """The case and its float64 reference, computed once and left unchanged:
    (case, dvp64, sums)."""
    import scan_ref as ref
    if cid not in _cache:
        b = dict(plain_cases() + [(f"frag_edges-{n}", lambda n=n: frag_edges(n)) for n in FRAG_EDGES_DIRECT]
                 + [(f"wide-{n}", lambda n=n: wide(n)) for n in WIDE])[cid]
        c = b()
        a = (c["rotP"], c["traP"], c["dat"], c["ctf"], c["sig"])
        _cache[cid] = (c, ref.dvp64(*a), ref.sums(*a))
    return _cache[cid]
