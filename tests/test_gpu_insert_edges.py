"""The three Fourier inserts (direct, tiled, binned), the CTF-search insert and
the gather against the float64 reference of scatter_ref.py, per voxel, at the
shapes where their kernels change path (insert_cases.py).

Every voxel must lie within its own rounding budget at the device's phase
margin P = 4 (scatter_ref.py derives it; test_scatter_ref.py measures the
oracle's share at P = 1), be exactly 0 outside the reference's support, and O
and the counter must match.  Every test asserts in numpy, before the kernel
runs, that its inputs reach the path it is named after.

Largest device err / budget (F.re, F.im, T) measured on an MI355X, next to
the oracle's in test_scatter_ref.py (the device's phase term is four times
the oracle's, so its ratios are the smaller ones where the phase dominates):

    case          direct           tiled            binned
    edge pf2 rU7  0.09 0.10 0.16   0.09 0.10 0.15   refused (radius)
    edge pf2 rU6  0.07 0.09 0.17   0.07 0.09 0.13   0.07 0.09 0.13
    edge pf1 rU6  0.06 0.05 0.11   0.06 0.05 0.13   refused (radius)
    edge pf1 rU5  0.03 0.03 0.11   0.04 0.03 0.08   0.03 0.03 0.08
    chunks        0.02 0.05 0.13   0.02 0.05 0.03   0.02 0.04 0.04
    many tiles    0.13 0.12 0.21   0.13 0.12 0.21   0.13 0.12 0.21
    grouping nC (1024, 0)  0.01 0.11 0.10   0.01 0.01 0.04   0.01 0.02 0.04
    grouping nC (1, 2000)  0.04 0.16 0.21   0.04 0.05 0.12   0.04 0.05 0.22
    mReco 1025 (tiled) 0.01 0.01 0.04      tiled paths 0.22 0.19 0.24
    non-finite (binned) 0.07 0.09 0.16
    CTF search: edge pf1 rU5 0.13 0.12 0.12, chunks (40) 0.17 0.21 0.24
    gather: 0.05 (pf 1 rU 6), 0.06 (pf 2 rU 7); adjoint identity 5e-8 relative
    (the default method repeats the figures of the method it picks)

Against a library whose kernels omit work -- the direct insert's grid stride,
the tiled insert's later z-chunks and its conjugation in the x = 0 cell, the
binned deposit's +1 row tap on a tile's last row and the group size in T --
the cases named after those paths fail and the others still pass.
"""
import numpy as np
import pytest
import torch

import insert_cases as ic
import scatter_ref as sr
from thunder_amd import ops
from thunder_amd._lib import ThxError, lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INS_CAP = 5120                      # insert.hip: LDS voxels of one tiled workgroup
PATCH_KC, PATCH_RT, PATCH_REC = 16, 128, 20     # patch.h

_cache = {}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _case(orc, name):
    """(case, float64 reference), built once per module."""
    if name not in _cache:
        build = {"edge_pf2_r7": lambda: ic.edge(orc, 2, 7), "edge_pf2_r6": lambda: ic.edge(orc, 2, 6),
                 "edge_pf1_r6": lambda: ic.edge(orc, 1, 6), "edge_pf1_r5": lambda: ic.edge(orc, 1, 5),
                 "chunks": lambda: ic.chunks(orc), "chunks40": lambda: ic.chunks(orc, mReco=40),
                 "many": lambda: ic.many(orc)}[name]
        c = build()
        _cache[name] = (c, _ref(c))
    return _cache[name]


def _ref(c, **kw):
    return sr.insert_f64(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"], c["w"],
                         c["px"], c["N"], **kw)


def _px(c):
    px = ops.PixelSet(c["N"], c["pf"], c["rU"], c["rL"], device=DEV)
    assert np.array_equal(px.iCol, c["px"].iCol) and np.array_equal(px.iRow, c["px"].iRow)
    return px


def _insert(c, method, nC=None):
    px = _px(c)
    hm = ops.HalfMap(c["vdim"], DEV)
    ops.insert3d(hm, T(c["dat"]), T(c["ctf"]), T(c["quat"]), T(c["trans"]), T(c["off"]), T(c["w"]), px,
                 method=method, nC=None if nC is None else T(np.asarray(nC, np.int32)))
    return hm, px


def _check(hm, ref, binned, label, skip=None):
    gF = hm.F.cpu().numpy().reshape(-1)
    gT = hm.T.cpu().numpy().reshape(-1)
    r = sr.check_insert(gF, gT, ref, P=4, binned=binned, skip=skip)
    print(f"{label}: device err / budget F.re {r[0]:.2f} F.im {r[1]:.2f} T {r[2]:.2f}")
    assert np.allclose(hm.O.cpu().numpy(), ref.O, rtol=1e-12, atol=1e-12)
    assert int(hm.counter.item()) == ref.cnt
    return r


def _precondition(name, c):
    x, y, z = sr.coords_f32(sr._mats(c["quat"][0]), c["px"].iCol, c["px"].iRow, c["pf"])
    if name.startswith("edge"):
        allc = np.concatenate([a.reshape(-1) for a in (x, y, z)])
        assert np.sum(allc == np.floor(allc)) > 100          # samples exactly on grid points
        assert np.sum((x > -1e-6) & (x < 0)) > 0              # a fold decided at 1e-16
        assert np.sum(x == 0) > 0                             # and samples on the x = 0 plane itself
    if name in ("edge_pf2_r7", "edge_pf1_r6"):                # the largest radius the front end admits
        assert c["rU"] * c["pf"] < c["vdim"] // 2 - 1 <= (c["rU"] + 1) * c["pf"]
    if name == "chunks":
        h, _ = ic.tile_histogram(c)
        assert h.max() > 2 * ic.BIN_E                         # a tile deposited in >= 3 chunks
    if name == "many":
        h, (R, ntx, nty, ntz) = ic.tile_histogram(c)
        order = ops.tile_order(c["px"].iCol, c["px"].iRow)
        assert c["px"].n > 4096                               # k_insert3d grid-strides
        assert len(order) > 2 * ic.BIN_KCH                    # >= 3 binning workgroups per image
        assert ntx * nty * ntz == 1372 > 1024                 # k_bin_scan's second pass with the carry
        assert np.count_nonzero(h[1024:]) > 0                 # and entries in tiles past the first pass


RUNS = [("edge_pf2_r7", "direct"), ("edge_pf2_r7", "tiled"), ("edge_pf2_r7", None),
        ("edge_pf2_r6", "direct"), ("edge_pf2_r6", "tiled"), ("edge_pf2_r6", "binned"), ("edge_pf2_r6", None),
        ("edge_pf1_r6", "direct"), ("edge_pf1_r6", "tiled"), ("edge_pf1_r6", None),
        ("edge_pf1_r5", "direct"), ("edge_pf1_r5", "tiled"), ("edge_pf1_r5", "binned"), ("edge_pf1_r5", None),
        ("chunks", "direct"), ("chunks", "tiled"), ("chunks", "binned"), ("chunks", None),
        ("many", "direct"), ("many", "tiled"), ("many", "binned"), ("many", None)]
# the front end's choice: binned where pf rU + 2 <= vdim / 2 - 1 (and mReco <= 1024), else tiled
DEFAULTS = {"edge_pf2_r7": "tiled", "edge_pf2_r6": "binned", "edge_pf1_r6": "tiled",
            "edge_pf1_r5": "binned", "chunks": "binned", "many": "binned"}


@pytest.mark.parametrize("name,method", RUNS)
def test_insert_per_voxel(orc, name, method):
    c, ref = _case(orc, name)
    _precondition(name, c)
    used = method
    if method is None:
        used = DEFAULTS[name]
        assert ops.insert_method(ops.HalfMap(c["vdim"], DEV), c["quat"].shape[1], _px(c)) == used
    hm, _ = _insert(c, method)
    _check(hm, ref, used == "binned", f"{name} {method or 'default'}")


@pytest.mark.parametrize("name", ["edge_pf2_r7", "edge_pf1_r6"])
def test_binned_refuses_the_edge_radius(orc, name):
    """pf rU + 2 > vdim / 2 - 1: the binned deposit's halo would leave the
    half-complex row; it returns its error and touches nothing."""
    c, _ = _case(orc, name)
    px = _px(c)
    hm = ops.HalfMap(c["vdim"], DEV)
    with pytest.raises(ThxError, match="reaches the volume edge"):
        ops.insert3d(hm, T(c["dat"]), T(c["ctf"]), T(c["quat"]), T(c["trans"]), T(c["off"]), T(c["w"]),
                     px, method="binned")
    assert not hm.F.any() and not hm.T.any() and int(hm.counter.item()) == 0


# ------------------------------------------------------------ grouping limit
@pytest.fixture(scope="module")
def grouped(orc):
    c = ic.grouping(orc)
    nq = [len(np.unique(q.view(np.uint64).reshape(-1, 4), axis=0)) for q in c["quat"]]
    assert c["quat"].shape[1] == ic.BIN_MAXM and max(nq) <= 60 and min(nq) > 30
    return c


@pytest.mark.parametrize("method", ["direct", "tiled", "binned"])
@pytest.mark.parametrize("nC", [(1024, 0), (1, 2000)])
def test_grouping_limit_and_sample_counts(orc, grouped, method, nC):
    """mReco = BIN_MAXM with resampled duplicates; nC of 0, 1, mReco and one
    above mReco, which clamps."""
    c = grouped
    key = ("grouping", nC)
    if key not in _cache:
        _cache[key] = _ref(c, nC=nC)
    ref = _cache[key]
    assert ref.cnt == sum(min(n, ic.BIN_MAXM) for n in nC)
    hm, _ = _insert(c, method, nC=nC)
    _check(hm, ref, method == "binned", f"grouping nC={nC} {method}")


def test_above_the_grouping_limit_falls_to_tiled(orc):
    c = ic.grouping(orc, mReco=ic.BIN_MAXM + 1)
    px = _px(c)
    hm = ops.HalfMap(c["vdim"], DEV)
    args = (T(c["dat"]), T(c["ctf"]), T(c["quat"]), T(c["trans"]), T(c["off"]), T(c["w"]), px)
    with pytest.raises(ThxError, match="mReco above 1024"):
        ops.insert3d(hm, *args, method="binned")
    assert not hm.F.any() and int(hm.counter.item()) == 0
    assert ops.insert_method(hm, ic.BIN_MAXM + 1, px) == "tiled"
    ops.insert3d(hm, *args)
    _check(hm, _ref(c), False, "grouping mReco=1025 default")


# --------------------------------------------------------------- tiled paths
def test_tiled_insert_takes_every_box_path(orc):
    from thunder_amd.ops import _ptr, _stream, workspace
    c = ic.tiled_paths(orc)
    ref = _ref(c)
    px = _px(c)
    nImg, mReco = c["quat"].shape[:2]
    hm = ops.HalfMap(c["vdim"], DEV)
    L = lib()
    ws = workspace(L.thx_insert3d_workspace(nImg, mReco, len(px.order)), DEV)
    d, cf, q, t, o, w = (T(c[k]) for k in ("dat", "ctf", "quat", "trans", "off", "w"))
    assert L.thx_insert3d_tiled(_ptr(hm.F), _ptr(hm.T), _ptr(hm.O), _ptr(hm.counter), hm.vdim, c["pf"],
                                _ptr(d), _ptr(cf), _ptr(q), _ptr(t), _ptr(o), _ptr(w), None, nImg, mReco,
                                _ptr(px.d_iCol), _ptr(px.d_iRow), _ptr(px.d_order), len(px.order), px.n,
                                px.idim, _ptr(ws), ws.numel(), _stream(DEV)) == 0, L.thx_last_error()
    torch.cuda.synchronize()
    nRec = nImg * ((mReco + PATCH_RT - 1) // PATCH_RT) * (len(px.order) // PATCH_KC)
    rec = ws[:nRec * PATCH_REC * 4].view(torch.int32).cpu().numpy().reshape(nRec, PATCH_REC).astype(np.int64)
    # k_insert_patches' path choice, restated from the record fields
    sp, nv0, nv1 = rec[:, 7], rec[:, 9], rec[:, 10] - rec[:, 9]
    sides = (nv0 > 0).astype(np.int64) + (nv1 > 0)
    live = sides > 0
    nz = np.where(live, np.maximum(nv0, nv1) // np.maximum(sp, 1), 0)
    zc = np.where(live, np.minimum(nz, INS_CAP // np.maximum(sp * sides, 1)), 0)
    fits, swept, direct = live & (zc == nz), live & (zc > 0) & (zc < nz), live & (zc == 0)
    both = (nv0 > 0) & (nv1 > 0)
    print(f"tiled paths: records {nRec} fit {fits.sum()} swept {swept.sum()} direct {direct.sum()} "
          f"both sides {both.sum()}")
    assert fits.sum() > 0 and swept.sum() > 0 and direct.sum() > 0 and both.sum() > 0
    _check(hm, ref, False, "tiled paths")


# ---------------------------------------------------------------- non-finite
def test_binned_insert_propagates_non_finite_pixels(orc):
    """One NaN and one Inf pixel in one image of a binned batch: the batch
    takes the float-atomic path; the non-finite voxels are the reference's,
    every other voxel stays within budget."""
    c0, _ = _case(orc, "edge_pf2_r6")
    c = dict(c0, dat=c0["dat"].copy())
    p = np.flatnonzero((c["px"].iCol > 0) & (c["px"].iRow != 0))
    c["dat"][1, p[3]] = np.nan
    c["dat"][1, p[11]] = complex(np.inf, 1.0)
    with np.errstate(invalid="ignore"):
        ref = _ref(c)
    bad = ~np.isfinite(ref.F)
    assert 0 < bad.sum() < ref.support.sum() / 2 and np.isfinite(ref.T).all()
    hm, _ = _insert(c, "binned")
    gF = hm.F.cpu().numpy().reshape(-1)
    assert np.array_equal(~np.isfinite(gF), bad)
    with np.errstate(invalid="ignore"):
        _check(hm, ref, True, "non-finite binned", skip=bad)
    gT = hm.T.cpu().numpy().reshape(-1)
    assert sr.worst(gT, ref.T, ref.bT(True)) <= 1


# ---------------------------------------------------------------- CTF search
@pytest.mark.parametrize("name", ["edge_pf1_r5", "chunks40"])
def test_ctf_search_insert_per_voxel(orc, name):
    c, _ = _case(orc, name)
    if name == "chunks40":
        h, _ = ic.tile_histogram(c)
        assert c["quat"].shape[1] == 40 and h.max() > 4000
    attr, nD = ic.ctf_search_inputs(c, 500)
    ref = _ref(dict(c, ctf=None), attr=attr, nD=nD)
    px = _px(c)
    hm = ops.HalfMap(c["vdim"], DEV)
    ops.insert3d_ctf(hm, T(c["dat"]), T(attr), T(nD), T(c["quat"]), T(c["trans"]), T(c["off"]),
                     T(c["w"]), px)
    _check(hm, ref, True, f"CTF search {name}")


# -------------------------------------------------------------------- gather
def _volume(vdim, seed):
    rng = np.random.default_rng(seed)
    shape = (vdim, vdim, vdim // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("name", ["edge_pf1_r6", "edge_pf2_r7"])
def test_gather_per_pixel(orc, name):
    """ops.project3d at pf 1, the edge radius and the on-grid rotations."""
    c, _ = _case(orc, name)
    _precondition(name, c)
    vol = _volume(c["vdim"], 9)
    mats = sr._mats(c["quat"][0])
    dmat = T(mats)
    P, b = sr.project_f64(vol, c["vdim"], c["pf"], mats, c["px"])
    got = ops.project3d(T(vol), dmat, _px(c)).cpu().numpy()
    r = max(sr.worst(got.real, P.real, b), sr.worst(got.imag, P.imag, b))
    print(f"gather {name}: device err / budget {r:.2f}")
    assert r <= 1


def test_device_insert_is_the_adjoint_of_the_device_gather(orc):
    """Re sum conj(project(V)) d = Re sum conj(V) insert(d) between the
    device's gather and its direct insert (unit CTF and weight, zero shift),
    evaluated in float64 on the host: the identity holds per tap, so only
    FP32 rounding separates the two sides."""
    c, _ = _case(orc, "edge_pf2_r7")
    nImg, mReco = c["quat"].shape[:2]
    px = _px(c)
    vol = _volume(c["vdim"], 11)
    proj = np.stack([ops.project3d(T(vol), ops.rotmat(T(c["quat"][l])), px).cpu().numpy()
                     for l in range(nImg)]).astype(np.complex128)          # [nImg, mReco, nPxl]
    # d = the mean projection of the image's samples + noise, so the sums do not cancel
    d = (proj.mean(1) + c["dat"]).astype(np.complex64)
    hm = ops.HalfMap(c["vdim"], DEV)
    ops.insert3d(hm, T(d), T(np.ones_like(c["ctf"])), T(c["quat"]), T(np.zeros_like(c["trans"])),
                 T(np.zeros_like(c["off"])), T(np.ones(nImg, np.float32)), px, method="direct")
    lhs = np.sum(np.conj(proj) * d.astype(np.complex128)[:, None, :]).real
    rhs = np.sum(np.conj(vol.astype(np.complex128)) * hm.F.cpu().numpy().astype(np.complex128)).real
    print(f"adjoint: lhs {lhs:.9g} rhs {rhs:.9g} rel {abs(lhs - rhs) / abs(rhs):.2e}")
    assert abs(rhs) > 100 and abs(lhs - rhs) <= 1e-5 * abs(rhs)
