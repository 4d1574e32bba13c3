"""The float64 reference of the 2D classification kernels (twod_ref.py)
against closed forms, its budgets against the FP32 emulations, every case's own
conditions (twod_cases.py), and the wrong restatements the comparison of
test_gpu_twod_edges.py must reject.  CPU only."""
import numpy as np
import pytest

import phase_ref as PR
import twod_cases as C
import twod_ref as R

# the largest emulation / budget share over the cases, as measured (DESIGN.md
# section 2); the test asserts the share is below 1 and at least a tenth of this
SHARE = {"gather": 0.815, "likelihood": 0.071}


# -------------------------------------------------------------- closed forms
def test_on_grid_rotations_permute_the_voxels():
    c, _, _ = C.get("fold-grid")
    img, vdim = c["img"], c["vdim"]
    X, Y = c["iCol"].astype(np.int64) * c["pf"], c["iRow"].astype(np.int64) * c["pf"]
    P = R.project2d_64(img, C.GRID, c["iCol"], c["iRow"], c["pf"])
    for r, (cs, sn) in enumerate(C.GRID.astype(np.int64)):
        x, y = cs * X - sn * Y, sn * X + cs * Y
        want = np.where(x < 0, np.conj(img[(-y) % vdim, np.abs(x)]), img[y % vdim, np.abs(x)])
        assert (P[r] == want).all()
    assert (R.emu_project2d_32(img, C.GRID, c["iCol"], c["iRow"], c["pf"]) == P.astype(np.complex64)).all()


@pytest.mark.parametrize("cid", ["ins-grid", "ins-pix-257"])
def test_gather_and_scatter_are_adjoint(cid):
    c, _ = C.get_insert(cid)
    rng = np.random.default_rng(5)
    vdim, nPxl = c["vdim"], c["dims"][2]
    img = rng.standard_normal((vdim, vdim // 2 + 1)) + 1j * rng.standard_normal((vdim, vdim // 2 + 1))
    a = rng.standard_normal(nPxl) + 1j * rng.standard_normal(nPxl)
    rot = c["rot"][:1]
    G = R.project2d_64(img, rot[0], c["iCol"], c["iRow"], c["pf"])                     # [m, i]
    z = np.zeros((1, rot.shape[1], 2))
    S = R.insert2d_64(vdim, c["pf"], a[None].astype(np.complex128), np.ones((1, nPxl), np.float32), rot, z,
                      np.zeros((1, 2)), np.ones(1, np.float32), None, c["iCol"], c["iRow"], c["idim"],
                      round32=False)
    # dat passes through complex64 in the insert: give both sides the rounded a
    a = a.astype(np.complex64).astype(np.complex128)
    lhs = (G * np.conj(a)[None, :]).real.sum()
    rhs = (img.reshape(-1) * np.conj(S.F)).real.sum()
    scale = (np.abs(G) * np.abs(a)[None, :]).sum()
    assert abs(lhs - rhs) <= 1e-13 * scale


def test_dvp_equals_a_literal_loop():
    c, d64, _ = C.get("cls-k")
    nImg, nR, nT, nPxl = c["dims"]
    vdim, pf, N = c["vdim"], c["pf"], c["idim"]
    for l in range(nImg):
        img = c["img"][c["cls"][l]]
        for r in range(nR):
            cs, sn = c["rot"][l, r]
            for t in range(nT):
                tx, ty = c["trans"][l, t]
                acc = 0.0
                for i in range(nPxl):
                    X, Y = float(c["iCol"][i] * pf), float(c["iRow"][i] * pf)
                    x, y = cs * X - sn * Y, sn * X + cs * Y
                    fold = not x >= 0
                    if fold:
                        x, y = -x, -y
                    x0, y0 = int(np.floor(x)), int(np.floor(y))
                    dx, dy = x - x0, y - y0
                    p = 0j
                    for j, wy in ((0, 1 - dy), (1, dy)):
                        for ii, wx in ((0, 1 - dx), (1, dx)):
                            row = y0 + j
                            p += complex(img[row if row >= 0 else row + vdim, x0 + ii]) * (wx * wy)
                    if fold:
                        p = p.conjugate()
                    ph = -2 * np.pi * (int(c["iCol"][i]) * tx + int(c["iRow"][i]) * ty) / N
                    e = complex(c["dat"][l, i]) - float(c["ctf"][l, i]) * complex(np.cos(ph), np.sin(ph)) * p
                    acc += float(c["sig"][l, i]) * (e.real ** 2 + e.imag ** 2)
                assert abs(acc - d64[l, r, t]) <= 1e-12 * abs(acc)


@pytest.mark.parametrize("cid", ["ins-pix-257", "ins-grid", "ins-cls"])
def test_insert_agrees_with_the_oracle(orc, cid):
    c, ref = C.get_insert(cid)
    px = orc.PixelSet(c["iCol"], c["iRow"], None, None, c["pf"])
    F, T, O, cnt = orc.insert2d_batch(c["vdim"], c["pf"], c["dat"], c["ctf"], c["rot"], c["trans"], c["off"],
                                      c["w"], c["nc"], px, c["idim"], nK=c["nK"])
    r = R.check_insert2d(F, T, O, cnt, ref, P=1)
    print(f"FIG {cid} oracle / budget F.re {r[0]:.3f} F.im {r[1]:.3f} T {r[2]:.3f} O {r[3]:.3f}")


def test_weights_bounds_hold_for_a_shifted_dvp():
    """A dvp moved by its whole budget, sample by sample in either direction,
    gives marginals inside weights2d_bounds."""
    for cid in ("cls-k", "cs-3x7"):
        c, d64, bud = C.get(cid)
        pri = (c["pC"], c["pR"], c["pT"]) + ((c["pD"],) if c["nD"] else ())
        ref = R.weights2d_64(d64, *pri)
        bounds = R.weights2d_bounds(d64, bud, *pri)
        sign = np.where(np.random.default_rng(3).random(d64.shape) < 0.5, -1.0, 1.0)
        got = R.weights2d_64(d64 + sign * bud, *pri)
        for g, w, b in zip(got, ref, bounds):
            assert (np.abs(g - w) <= b).all()


# ------------------------------------------------------------------- budgets
def test_emulations_stay_inside_the_budgets():
    top = {"gather": 0.0, "likelihood": 0.0}
    for cid in C.LOCAL:
        c, d64, bud = C.get(cid)
        assert (bud > 0).all() and np.isfinite(bud).all()
        s = R.worst(R.emu_local2d_32(*C.args(c)), d64, bud)
        print(f"FIG {cid} emulation / budget {s:.3f}")
        top["likelihood"] = max(top["likelihood"], s)
    for cid in C.proj_cases():
        img, rot, iCol, iRow, pf, _ = C.get_proj(cid)
        P, Pa, D, L1 = R.project2d_64(img, rot, iCol, iRow, pf, extras=True)
        s = R.worst(R.emu_project2d_32(img, rot, iCol, iRow, pf), P, R.gather_budget(Pa, D, L1))
        print(f"FIG {cid} gather emulation / budget {s:.3f}")
        top["gather"] = max(top["gather"], s)
    print("FIG largest emulation / budget " + " ".join(f"{k} {v:.3f}" for k, v in top.items()))
    for k, v in top.items():
        assert v < 1.0, f"{k}: the emulation leaves its budget ({v:.3f})"
        assert v >= SHARE[k] / 10, f"{k}: the budget is vacuous (share {v:.4f})"


# ---------------------------------------------------------------- conditions
def _coords(c, rot=None):
    return R.coords2_64(c["rot"] if rot is None else rot, c["iCol"], c["iRow"], c["pf"])


def _common(rot, iCol, iRow, pf, vdim):
    x, y = R.coords2_64(rot, iCol, iRow, pf)
    assert R.taps_in_range(x, y, vdim)
    assert R.taps_in_range(x.astype(np.float32), y.astype(np.float32), vdim)
    assert C.rot_ok(rot, iCol, iRow, pf).all(), "fused and unfused coordinates may decide apart"
    # the FP32 rounding keeps the cell and the fold of the FP64 coordinate
    a, b = R.cell2(x, y), R.cell2(x.astype(np.float32), y.astype(np.float32))
    assert (a[0] == b[0]).all() and all((p == q).all() for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("cid", C.LOCAL)
def test_local_case_conditions(cid):
    c, d64, bud = C.get(cid)
    nImg, nR, nT, nPxl = c["dims"]
    _common(c["rot"], c["iCol"], c["iRow"], c["pf"], c["vdim"])
    assert C.hermitian_x0(c["img"])
    assert (c["sig"] < 0).all() and c["dat"].shape == (nImg, nPxl)
    if nPxl >= 16:
        assert (c["ctf"] > 0).any() and (c["ctf"] < 0).any()
    assert nImg == 1 or len(set(c["pC"])) == nImg
    assert nImg <= 4
    nCol = nT * max(c["nD"], 1)
    name, _, arg = cid.partition("-")
    if name == "pix":
        assert nPxl == int(arg)
    if name == "col":
        assert nT == int(arg) and not c["nD"]
    if name == "cs":
        assert c["ctfD"].shape == (nImg, c["nD"], nPxl) and nCol <= 1024
    vox = (c["vdim"] // 2 + 1) * c["vdim"]
    staged = vox <= 18432
    assert staged == (not cid.startswith("global"))
    x, y = (a.astype(np.float32) for a in _coords(c))
    conj, (x0, y0), _ = R.cell2(x, y)
    if cid in ("col-17", "col-33", "cs-1x17"):
        assert nCol % R.TMAX == 1                       # the last column pass holds one column
    if cid in ("col-16", "col-32", "cs-16x2", "cs-8x4", "cs-64x16"):
        assert nCol % R.TMAX == 0
    if cid in ("cs-3x7", "cs-1x17", "cs-65x3"):
        assert R.TMAX % c["nD"] != 0 and nCol > R.TMAX    # a pass boundary inside a defocus group
    if cid == "cs-65x3":
        assert nT > 64
    if cid == "cs-64x16":
        assert nCol == 1024 and nR == 1 and nPxl == 16
    if cid == "rot-1":
        assert nR == 1
    if cid == "rot-dup":
        assert (c["rot"][:, 0] == c["rot"][:, 1]).all()
    if cid == "fold-grid":
        assert (c["rot"][:, :4] == C.GRID).all()
        for a in (x, y):
            assert (a[:, :4] == np.rint(a[:, :4])).all()
        zero = x == 0
        assert (zero & ~np.signbit(x)).any() and (zero & np.signbit(x)).any(), "needs x = +0.0 and -0.0"
        assert ((c["iCol"] == 0) & (c["iRow"] < 0)).any() and (c["iRow"] == 0).any()
        assert (y0[:, :4] < 0).any() and (conj[:, :4]).any() and (~conj[:, :4]).any()
        assert ((x > -1) & (x < 0)).any() and ((x > 0) & (x < 1)).any(), "no cell straddles x = 0"
    if cid == "edge-ring":
        h = c["vdim"] // 2
        assert (x0 + 1 == h).any() and (y0 + 1 == h).any() and (y0 == -h).any()
    if cid.startswith("lds-190"):
        assert c["vdim"] == 190 and vox * 8 == 145920
    if cid.startswith("global-192"):
        assert c["vdim"] == 192
    if cid in ("lds-190-k", "global-192-k"):
        assert c["nK"] == 3 and c["cls"][0] == 2 and len(set(c["cls"])) == 2
    if cid == "cls-k":
        assert set(c["cls"]) == {0, 1, 2} and c["cls"][0] != 0
    if cid == "cls-null":
        assert nImg == 1 and c["cls"] is None


@pytest.mark.parametrize("cid", C.INSERT)
def test_insert_case_conditions(cid):
    c, ref = C.get_insert(cid)
    nImg, mReco, nPxl = c["dims"]
    _common(c["rot"], c["iCol"], c["iRow"], c["pf"], c["vdim"])
    assert (c["ctf"] > 0).any() and (c["ctf"] < 0).any() or nPxl == 1
    if cid.startswith("ins-pix-"):
        assert nPxl == int(cid.rsplit("-", 1)[1])
    x, y = (a.astype(np.float32) for a in _coords(c))
    conj, (x0, y0), (fx, fy) = R.cell2(x, y)
    if cid == "ins-grid":
        on = (fx == 0) & (fy == 0)
        assert on[:, :4].all() and (on & (x0 == 0) & conj).sum() == 0
        assert ((x == 0) & (y != 0)).any()
        assert ((x0 == 0) & conj).any() and ((x0 == 0) & ~conj).any()
    if cid == "ins-cls":
        assert c["nK"] == 4 and set(c["nc"].reshape(-1)) == {0, 1, 3}
        assert (c["nc"][:, 1:] != c["nc"][:, :1]).any(1).all()
        assert ref.cnt[2] == 0 and ref.cnt[3] > 0
        size = (c["vdim"] // 2 + 1) * c["vdim"]
        assert not ref.n[2 * size:3 * size].any()
    if cid.startswith("ins-d"):
        assert c["attr"].shape == (nImg, 8) and c["nD"].shape == (nImg, mReco)


def test_projection_and_scan_case_conditions():
    img, rot, iCol, iRow, pf, vdim = C.get_proj("proj-cap")
    assert len(iCol) == 8193 and len(rot) == 2 and vdim == 160 and pf == 1
    _common(rot, iCol, iRow, pf, vdim)
    assert C.hermitian_x0(img)
    for cid, (nPxl, nR, nT) in C.G2D.items():
        c = C.get_g2d(cid)
        assert c["dims"] == (3, nR, nT, nPxl) and c["nK"] == 3
        _common(c["rot"], c["iCol"], c["iRow"], c["pf"], c["vdim"])


# ----------------------------------------------------------------- mutations
def _factor(tag, mut, ref, bud):
    f = R.worst(mut, ref, bud)
    print(f"FIG mutation {tag}: error / budget {f:.3g}")
    return f


def _dvp_mut(cid, mut):
    c, d64, bud = C.get(cid)
    return _factor(f"{mut} ({cid})", R.dvp2d_64(*C.args(c), P=c["P"], mut=mut), d64, bud)


def _proj_mut(cid, mut):
    img, rot, iCol, iRow, pf, _ = C.get_proj(cid)
    P, Pa, D, L1 = R.project2d_64(img, rot, iCol, iRow, pf, extras=True)
    return _factor(f"gather {mut} ({cid})", R.project2d_64(img, rot, iCol, iRow, pf, mut=mut), P,
                   R.gather_budget(Pa, D, L1))


def test_the_likelihood_budget_rejects_wrong_restatements():
    assert _dvp_mut("fold-grid", "noconj") > 1 and _proj_mut("fold-grid", "noconj") > 1
    assert _dvp_mut("fold-grid", "nowrap") > 1 and _proj_mut("fold-grid", "nowrap") > 1
    assert _dvp_mut("edge-ring", "nowrap") > 1
    assert _dvp_mut("pix-65", "tap11") > 1 and _proj_mut("pix-257", "tap11") > 1
    for n in C.PIX:
        assert _dvp_mut(f"pix-{n}", "droplast") > 1
    for cid in ("pix-257", "pix-513"):
        assert _dvp_mut(cid, "drop256") > 1
    for cid in ("col-17", "col-32", "col-33", "cs-3x7", "cs-16x2", "cs-8x4", "cs-1x17", "cs-65x3", "cs-64x16"):
        assert _dvp_mut(cid, "droplastcol") > 1
    for cid in ("cs-5x3", "cs-3x7", "cs-16x2", "cs-65x3"):
        assert _dvp_mut(cid, "colorder") > 1
    for cid in C.SEARCH:
        assert _dvp_mut(cid, "ctfd0") > 1
    for cid in ("cls-k", "lds-190-k", "global-192-k"):
        assert _dvp_mut(cid, "cls0") > 1
    for cid in ("col-1", "pix-1", "pix-65"):
        assert _dvp_mut(cid, "transsign") > 1


def test_fold_at_zero_cannot_be_told_apart_in_the_gather():
    """Fold decided by x > 0 differs from !(x >= 0) only at x = +-0, where the
    sample is an exact grid point of the x = 0 column: on a Hermitian column
    the folded read is the conjugate of the mirrored voxel, the same number.
    The gather cannot see it (the insert does, below)."""
    c, d64, _ = C.get("fold-grid")
    assert (R.dvp2d_64(*C.args(c), mut="foldgt") == d64).all()


def test_the_insert_budget_rejects_wrong_restatements():
    def rejected(cid, mut):
        c, ref = C.get_insert(cid)
        bad = R.insert2d_64(*C.insert_args(c), nK=c["nK"], attr=c["attr"], nD=c["nD"], mut=mut)
        with pytest.raises(AssertionError):
            R.check_insert2d(bad.F, bad.T, bad.O, bad.cnt, ref, P=R.P_HW)

    for cid in ("ins-grid", "ins-pix-257"):
        rejected(cid, "noconj")
    rejected("ins-grid", "foldgt")
    for cid in ("ins-pix-1", "ins-cls", "ins-d"):
        rejected(cid, "osign")
        rejected(cid, "tctf")
    rejected("ins-cls", "clsfirst")
    rejected("ins-d-cls", "clsfirst")
    # the reference passes its own check, and twice the insert the doubled one
    for cid in C.INSERT:
        c, ref = C.get_insert(cid)
        R.check_insert2d(ref.F, ref.T, ref.O, ref.cnt, ref, P=R.P_HW)
        two = R.scaled(ref, 2)
        R.check_insert2d(2 * ref.F, 2 * ref.T, 2 * ref.O, 2 * ref.cnt, two, P=R.P_HW)


def test_marginal_bounds_reject_a_wrong_prior():
    c, d64, bud = C.get("cls-k")
    ref = R.weights2d_64(d64, c["pC"], c["pR"], c["pT"])
    bounds = R.weights2d_bounds(d64, bud, c["pC"], c["pR"], c["pT"])
    flat = np.broadcast_to(c["pR"].mean(1, keepdims=True), c["pR"].shape)
    bad = R.weights2d_64(d64, c["pC"], flat, c["pT"])
    assert R.worst(bad[2], ref[2], bounds[2]) > 1
    assert PR.worst(ref[1], ref[1], bounds[1]) == 0
