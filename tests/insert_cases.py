"""Seeded edge cases of the Fourier insert, shared by the CPU check of the
oracle (test_scatter_ref.py) and the device check (test_gpu_insert_edges.py).

Inputs: dat complex normal, ctf = +-10^U(-3, 0), shifts with sigma 3 px
(6 px in the many-tiles case), offsets with sigma 1 px."""
import numpy as np

from thunder_amd import synth

S = np.sqrt(0.5)
ON_GRID = np.array([(1, 0, 0, 0), (S, 0, 0, S), (0, 0, 0, 1), (0, 1, 0, 0), (0, 0, 1, 0),
                    (S, S, 0, 0), (S, 0, S, 0), (.5, .5, .5, .5)], np.float64)

BIN_E, BIN_KCH, BIN_MAXM, BT = 32768, 2048, 1024, 16     # insert_binned.hip


def inputs(orc, N, pf, rU, rL, quat, seed, shift=3.0):
    rng = np.random.default_rng(seed)
    px = orc.pixel_set(N, pf, rU, rL)
    nImg, mReco = quat.shape[:2]
    dat = (rng.standard_normal((nImg, px.n)) + 1j * rng.standard_normal((nImg, px.n))).astype(np.complex64)
    ctf = (10.0 ** rng.uniform(-3, 0, (nImg, px.n)) * rng.choice([-1.0, 1.0], (nImg, px.n))).astype(np.float32)
    trans = rng.standard_normal((nImg, mReco, 2)) * shift
    off = rng.standard_normal((nImg, 2))
    w = (rng.uniform(0.5, 1.5, nImg) / mReco).astype(np.float32)
    return dict(N=N, pf=pf, rU=rU, rL=rL, vdim=N * pf, px=px, dat=dat, ctf=ctf,
                quat=np.ascontiguousarray(quat), trans=trans, off=off, w=w, nC=None)


def edge(orc, pf, rU, seed=100):
    """N 16, rL 0, 2 images x (the eight on-grid rotations + 8 uniform ones)."""
    rng = np.random.default_rng(seed + 7)
    quat = np.stack([np.concatenate([ON_GRID, synth.uniform_quaternions(8, rng)]) for _ in range(2)])
    return inputs(orc, 16, pf, rU, 0, quat, seed)


def chunks(orc, mReco=400, seed=200):
    """N 32, pf 2, rU 8, rL 1: 6 images x mReco distinct rotations, every
    image's cloud 1 degree around one shared pose, so the same few tiles take
    all the entries."""
    rng = np.random.default_rng(seed + 7)
    one = synth.clustered_quaternions(1, 6 * mReco, 1.0, rng)
    return inputs(orc, 32, 2, 8, 1, one.reshape(6, mReco, 4), seed)


def grouping(orc, mReco=BIN_MAXM, seed=300):
    """N 16, pf 2, rU 5, 2 images x mReco samples drawn (with repeats, as a
    resampled particle) from 60 ancestors at 3 degrees."""
    rng = np.random.default_rng(seed + 7)
    anc = synth.clustered_quaternions(2, 60, 3.0, rng)
    pick = rng.integers(0, 60, (2, mReco))
    quat = np.stack([anc[l][pick[l]] for l in range(2)])
    return inputs(orc, 16, 2, 5, 0, quat, seed)


def many(orc, seed=400):
    """N 112, pf 2, rU 54, rL 0: 2 images x 6 samples at 3 degrees, shifts sigma 6 px."""
    rng = np.random.default_rng(seed + 7)
    return inputs(orc, 112, 2, 54, 0, synth.clustered_quaternions(2, 6, 3.0, rng), seed, shift=6.0)


def tiled_paths(orc, seed=700):
    """N 64, pf 2, rU 30, rL 0, 3 images x 24 samples (one record tile each):
    image 0's cloud at 1 degree (patch boxes that fit the tiled insert's LDS),
    image 1's at 12 degrees (boxes swept in z-chunks), image 2's rotations
    uniform (outer patches whose single slice pair does not fit)."""
    rng = np.random.default_rng(seed + 7)
    quat = np.concatenate([synth.clustered_quaternions(1, 24, 1.0, rng),
                           synth.clustered_quaternions(1, 24, 12.0, rng),
                           synth.uniform_quaternions(24, rng)[None]])
    return inputs(orc, 64, 2, 30, 0, quat, seed)


def tile_histogram(case):
    """Entries (distinct rotation of an image, pixel) per 16^3-corner tile of
    the binned deposit's grid: (counts [nt], grid (R, ntx, nty, ntz))."""
    from scatter_ref import _mats, coords_f32, fold_taps
    pf, rMax = case["pf"], int(np.ceil(case["rU"]))
    R = pf * rMax + 2
    ntx, nty = (R + BT - 1) // BT, (2 * R + BT - 1) // BT
    cnt = np.zeros(ntx * nty * nty, np.int64)
    for q in case["quat"]:
        uq = np.unique(q.view(np.uint64).reshape(len(q), 4), axis=0).view(np.float64)
        x, y, z = coords_f32(_mats(uq), case["px"].iCol, case["px"].iRow, pf)
        _, _, _, (x0, y0, z0) = fold_taps(x, y, z, case["vdim"])
        t = (((z0 + R) // BT) * nty + (y0 + R) // BT) * ntx + x0 // BT
        np.add.at(cnt, t.reshape(-1), 1)
    return cnt, (R, ntx, nty, nty)


def ctf_search_inputs(case, seed):
    """attr [nImg, 8] and defocus factors nD [nImg, mReco] ~ N(1, 0.02) for a case."""
    nImg, mReco = case["quat"].shape[:2]
    rng = np.random.default_rng(seed)
    return synth.ctf_attrs(nImg, seed=seed + 1), 1.0 + 0.02 * rng.standard_normal((nImg, mReco))
