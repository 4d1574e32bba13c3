"""The 2D classification kernels (csrc/twod.hip) at their edges, against the
float64 reference and the absolute budgets of twod_ref.py (DESIGN.md section
2), on the cases of twod_cases.py.  Every case runs through every entry point
that reaches its kernel:

  k_local2d    thx_local_phase2d (dvp dump, and dvp NULL + workspace),
               thx_local_phase2d_d (the cs-* cases; every plain case at nD 1
               with pD = [1], bit-identical dvp), and two cases through
               ExpectLocalV2D / RTD / PreI2D / M (4-double rotation rows)
  k_project2d  thx_project2d, and thx_ExpectGlobal2D (project + global scan)
  k_insert2d   thx_insert2d, thx_insert2d_d, thx_InsertI2D

Per local case: three calls -- every output, the dump and the workspace filled
with NaN, with 1e30, with NaN again -- give bit-identical results; every dvp
sample within dvp_budget of dvp2d_64; the baseline exactly the dump's maximum;
every marginal entry finite, >= 0 and within weights2d_bounds (no
share-of-maximum floor).  Every tap of every case is asserted in range on the
CPU (twod_cases / twod_ref) before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import phase_ref as PR
import scan_ref as SR
import twod_cases as C
import twod_ref as R
from thunder_amd import ops
from thunder_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
p = ops._ptr


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def full(fill, *shape, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=DEV)


_dev = {}


def up(cid):
    if cid not in _dev:
        c, _, _ = C.get(cid)
        x, y = R.coords2_64(c["rot"], c["iCol"], c["iRow"], c["pf"])
        assert R.taps_in_range(x.astype(np.float32), y.astype(np.float32), c["vdim"])
        g = {k: t(c[k]) for k in ("img", "rot", "trans", "dat", "ctf", "sig", "pC", "pR", "pT", "iCol", "iRow")}
        if c["nD"]:
            g.update(ctfD=t(c["ctfD"]), pD=t(c["pD"]))
        g["cls"] = t(c["cls"]) if c["cls"] is not None else None
        g["one"] = torch.ones(c["dims"][0], 1, dtype=torch.float64, device=DEV)
        _dev[cid] = g
    return _dev[cid]


def local(cid, fill=float("nan"), want_dvp=True, search=None, cls="own", ws_short=0, vdim=None, over=None):
    """One call of thx_local_phase2d (search False) or thx_local_phase2d_d
    through ctypes; every output, the dump and the workspace hold `fill` on
    entry.  search on a plain case: nD 1, pD = [1], ctfD = ctf.  over:
    (nT, nD) of a refused size.  -> (status, dict of numpy outputs)."""
    c, _, _ = C.get(cid)
    g = up(cid)
    nImg, nR, nT, nPxl = c["dims"]
    search = bool(c["nD"]) if search is None else search
    nD = (c["nD"] or 1) if search else 0
    trans, pT, pD, ctf = g["trans"], g["pT"], g.get("pD", g["one"]), g["ctfD"] if c["nD"] else g["ctf"]
    if over:
        nT, nD = over
        trans, pT = torch.zeros(nImg, nT, 2, dtype=torch.float64, device=DEV), full(1.0 / nT, nImg, nT, dtype=torch.float64)
        pD, ctf = full(1.0 / nD, nImg, nD, dtype=torch.float64), torch.zeros(nImg, nD, nPxl, device=DEV)
    nCol = nT * max(nD, 1)
    out = dict(wC=full(fill, nImg), wR=full(fill, nImg, nR), wT=full(fill, nImg, nT))
    if search:
        out["wD"] = full(fill, nImg, nD)
    out["base"] = full(fill, nImg)
    out["dvp"] = full(fill, nImg, nR, nCol) if want_dvp else None
    L = lib()
    need = L.thx_local_phase2d_d_workspace(nImg, nR, nT, nD) if search else L.thx_local_phase2d_workspace(nImg, nR, nT)
    ws = full(fill, (need + 3) // 4)
    cl = g["cls"] if isinstance(cls, str) else cls
    head = (p(g["img"]), c["vdim"] if vdim is None else vdim, c["pf"], p(cl), p(g["rot"]), nR, p(trans), nT)
    img = (p(g["dat"]), p(ctf), p(g["sig"]), p(g["iCol"]), p(g["iRow"]), nPxl, c["idim"], nImg)
    tail = (p(out["base"]), p(out["dvp"]), p(ws), need - ws_short, ops._stream(torch.device(DEV)))
    if search:
        st = L.thx_local_phase2d_d(*head, nD, p(g["pC"]), p(g["pR"]), p(pT), p(pD), *img, p(out["wC"]), p(out["wR"]),
                                   p(out["wT"]), p(out["wD"]), *tail)
    else:
        st = L.thx_local_phase2d(*head, p(g["pC"]), p(g["pR"]), p(pT), *img, p(out["wC"]), p(out["wR"]),
                                 p(out["wT"]), *tail)
    torch.cuda.synchronize()
    return st, {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def same_bits(a, b, keys=None):
    return all(a[k].shape == b[k].shape and (a[k].view(np.int32) == b[k].view(np.int32)).all()
               for k in (a if keys is None else keys))


def three_calls(cid, **kw):
    outs = []
    for fill in (float("nan"), BIG, float("nan")):
        st, o = local(cid, fill=fill, **kw)
        assert st == 0, lib().thx_last_error()
        outs.append(o)
    assert same_bits(outs[0], outs[1]), "outputs depend on what the buffers held"
    assert same_bits(outs[0], outs[2]), "outputs differ between two identical calls"
    return outs[0]


def check_marginals(tag, got, ref, bounds):
    w = {}
    for name, g_, r, b in zip(("wC", "wR", "wT", "wD"), got, ref, bounds):
        assert np.isfinite(g_).all() and (g_ >= 0).all(), f"{tag} {name}: not finite or negative"
        w[name] = R.worst(g_, r, b)
    print(f"FIG {tag} marginals / bound " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, f"{tag}: marginal error / bound {w}"


def check_local(cid, out, tag):
    c, d64, bud = C.get(cid)
    nImg = c["dims"][0]
    ratio = R.worst(out["dvp"], d64, bud)
    branch = "global" if cid.startswith("global") else "staged"
    print(f"FIG {tag} dvp / budget ({branch}) {ratio:.3f}")
    assert ratio <= 1.0, f"{tag}: largest dvp error / budget {ratio:.3f}"
    assert (out["base"] == out["dvp"].reshape(nImg, -1).max(1)).all(), f"{tag}: baseline is not the dump's maximum"
    search = "wD" in out
    pD = (c["pD"] if c["nD"] else np.ones((nImg, 1))) if search else None
    pri = (c["pC"], c["pR"], c["pT"]) + ((pD,) if search else ())
    ref = R.weights2d_64(d64, *pri)
    bounds = R.weights2d_bounds(d64, bud, *pri)
    check_marginals(tag, [out[k] for k in (("wC", "wR", "wT", "wD") if search else ("wC", "wR", "wT"))], ref, bounds)


# --------------------------------------------------------------- local phase
@pytest.mark.parametrize("cid", C.PLAIN)
def test_local_phase2d(cid):
    out = three_calls(cid)
    check_local(cid, out, f"{cid} plain")
    st, bare = local(cid, want_dvp=False)
    assert st == 0 and same_bits(out, bare, bare), "the weights depend on the dump"
    # nD 1 with pD = [1] through the search entry: the same dvp bit for bit
    st, d1 = local(cid, search=True)
    assert st == 0, lib().thx_last_error()
    assert same_bits(out, d1, ["dvp", "base"])
    check_local(cid, d1, f"{cid} d(nD 1)")
    if cid == "rot-dup":
        assert (out["dvp"][:, 0].view(np.int32) == out["dvp"][:, 1].view(np.int32)).all()
        assert (out["wR"][:, 0].view(np.int32) == out["wR"][:, 1].view(np.int32)).all()
    if cid == "cls-null":
        st, z = local(cid, cls=torch.zeros(1, dtype=torch.int32, device=DEV))
        assert st == 0 and same_bits(out, z), "cls NULL and cls all zero differ"


@pytest.mark.parametrize("cid", C.SEARCH)
def test_local_phase2d_d(cid):
    out = three_calls(cid)
    check_local(cid, out, f"{cid} d")
    st, bare = local(cid, want_dvp=False)
    assert st == 0 and same_bits(out, bare, bare), "the weights depend on the dump"


def test_local_refusals():
    """Each returns an error and leaves every output, the dump and the
    workspace's contents untouched; the next valid call is unaffected."""
    good = three_calls("col-17")
    good_d = three_calls("cs-5x3")

    def refused(cid, **kw):
        st, o = local(cid, **kw)
        assert st != 0, f"{kw} was accepted"
        assert all(np.isnan(v).all() for v in o.values()), f"{kw}: an output was written"

    refused("col-17", want_dvp=False, ws_short=1)
    refused("cs-5x3", want_dvp=False, ws_short=1)
    refused("col-17", vdim=31)
    refused("cs-5x3", vdim=31)
    refused("cs-5x3", over=(205, 5))                  # nT nD = 1025
    refused("cs-5x3", over=(1025, 1))
    assert same_bits(three_calls("col-17"), good) and same_bits(three_calls("cs-5x3"), good_d)


@pytest.mark.parametrize("cid", ["col-17", "fold-grid"])
def test_local_per_image_surface(cid):
    """ExpectLocalV2D -> ExpectLocalRTD (4-double rotation rows) ->
    ExpectLocalPreI2D -> ExpectLocalM, one image at a time."""
    c, d64, bud = C.get(cid)
    up(cid)                                            # the tap range check
    nImg, mR, mT, npxl = c["dims"]
    vdim, pf, N = c["vdim"], c["pf"], c["idim"]
    L, vp, gpu, cpy = lib(), ctypes.c_void_p, 0, 2
    P = lambda a: a.ctypes.data_as(vp)
    iCol, iRow = np.ascontiguousarray(c["iCol"], np.int32), np.ascontiguousarray(c["iRow"], np.int32)
    dCol, dRow, mgr, mcp = vp(), vp(), vp(), vp()
    assert L.thx_ExpectPreidx(gpu, ctypes.byref(dCol), ctypes.byref(dRow), P(iCol), P(iRow), npxl) == 0
    assert L.thx_tex_create(0, vdim, gpu, ctypes.byref(mgr)) == 0
    dat = np.ascontiguousarray(c["dat"]).view(np.float32)
    ctf, sig = np.ascontiguousarray(c["ctf"]), np.ascontiguousarray(c["sig"])
    dD, dC, dO, dS = vp(), vp(), vp(), vp()
    assert L.thx_ExpectLocalIn(gpu, ctypes.byref(dD), ctypes.byref(dC), ctypes.byref(dO), ctypes.byref(dS),
                               npxl, cpy, 1) == 0
    assert L.thx_calpoint_create(0, 1, gpu, mR, mT, 1, npxl, ctypes.byref(mcp)) == 0
    cl = np.ascontiguousarray(c["img"]).view(np.float32)
    got = [np.full((nImg, n), np.nan, np.float32) for n in (1, mR, mT)]
    for l in range(nImg):
        assert L.thx_ExpectLocalV2D(gpu, mgr, P(cl), (vdim // 2 + 1) * vdim) == 0, L.thx_last_error()
        slot = l % cpy
        assert L.thx_ExpectLocalP(gpu, dD, dC, dO, dS, P(dat), P(ctf), None, P(sig), slot, l, npxl, 0) == 0
        rot4 = np.zeros((mR, 4))
        rot4[:, :2] = c["rot"][l]
        tr = np.ascontiguousarray(c["trans"][l])
        pR, pT = np.ascontiguousarray(c["pR"][l]), np.ascontiguousarray(c["pT"][l])
        oldD, dpara = np.ones(1), np.ones(1)
        assert L.thx_ExpectLocalRTD(gpu, mcp, P(pR), P(pT), P(oldD), P(tr), P(rot4), P(dpara)) == 0
        assert L.thx_ExpectLocalPreI2D(gpu, slot, mgr, mcp, None, None, dCol, dRow, 0.0, 0.1, 0.0, 0.0, pf, N,
                                       vdim, npxl, 1) == 0, L.thx_last_error()
        wC, wR, wT, wD = (np.full(n, np.nan, np.float32) for n in (1, mR, mT, 1))
        assert L.thx_ExpectLocalM(gpu, slot, mcp, dD, dC, dS, P(wC), P(wR), P(wT), P(wD), float(c["pC"][l]),
                                  npxl) == 0, L.thx_last_error()
        got[0][l], got[1][l], got[2][l] = wC, wR, wT
    assert L.thx_calpoint_destroy(mcp) == 0
    assert L.thx_ExpectLocalFin(gpu, ctypes.byref(dD), ctypes.byref(dC), ctypes.byref(dO), None,
                                ctypes.byref(dS), 0) == 0
    assert L.thx_tex_destroy(mgr) == 0
    assert L.thx_ExpectFreeIdx(gpu, ctypes.byref(dCol), ctypes.byref(dRow)) == 0
    ref = R.weights2d_64(d64, c["pC"], c["pR"], c["pT"])
    bounds = R.weights2d_bounds(d64, bud, c["pC"], c["pR"], c["pT"])
    check_marginals(f"{cid} per-image", [got[0][:, 0], got[1], got[2]], ref, bounds)


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("cid", C.proj_cases())
def test_project2d(cid):
    img, rot, iCol, iRow, pf, vdim = C.get_proj(cid)
    P64, Pa, D, L1 = R.project2d_64(img, rot, iCol, iRow, pf, extras=True)      # asserts the tap range
    x, y = R.coords2_64(rot, iCol, iRow, pf)
    assert R.taps_in_range(x.astype(np.float32), y.astype(np.float32), vdim)
    nR, nPxl = P64.shape
    g = [t(a) for a in (img, rot, iCol, iRow)]
    outs = []
    for fill in (float("nan"), BIG):
        o = torch.view_as_complex(full(fill, nR, nPxl, 2))
        st = lib().thx_project2d(p(g[0]), vdim, pf, p(g[1]), nR, p(g[2]), p(g[3]), nPxl, p(o), None)
        assert st == 0, lib().thx_last_error()
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
    assert (outs[0].view(np.int32) == outs[1].view(np.int32)).all(), "an output was left unwritten"
    ratio = R.worst(outs[0], P64, R.gather_budget(Pa, D, L1))
    print(f"FIG {cid} gather / budget {ratio:.3f}")
    assert ratio <= 1.0
    if cid == "fold-grid":
        assert (rot[:4] == C.GRID).all()
        assert (outs[0][:4].view(np.int32) == P64[:4].astype(np.complex64).view(np.int32)).all()
    # nR 0 and nPxl 0 return OK without touching the output
    for n_r, n_p in ((0, nPxl), (nR, 0)):
        o = full(float("nan"), nR, nPxl, 2)
        assert lib().thx_project2d(p(g[0]), vdim, pf, p(g[1]), n_r, p(g[2]), p(g[3]), n_p, p(o), None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all())


# -------------------------------------------------------------------- insert
def maps(c):
    size = (c["vdim"] // 2 + 1) * c["vdim"]
    nK = c["nK"]
    return (torch.zeros(nK * size, 2, device=DEV), torch.zeros(nK * size, device=DEV),
            torch.zeros(nK, 2, dtype=torch.float64, device=DEV), torch.zeros(nK, dtype=torch.int32, device=DEV))


def insert(c, m, nc="own"):
    nImg, mReco, nPxl = c["dims"]
    a = {k: t(c[k]) for k in ("dat", "rot", "trans", "off", "w", "iCol", "iRow")}
    ncd = (t(c["nc"]) if c["nc"] is not None else None) if isinstance(nc, str) else nc
    F, T, O, cnt = m
    tail = (p(a["rot"]), p(a["trans"]), p(a["off"]), p(a["w"]), p(ncd), nImg, mReco, p(a["iCol"]), p(a["iRow"]),
            nPxl, c["idim"], None)
    if c["attr"] is not None:
        attr, nD = t(np.asarray(c["attr"], np.float32)), t(np.asarray(c["nD"], np.float64))
        st = lib().thx_insert2d_d(p(F), p(T), p(O), p(cnt), c["vdim"], c["pf"], p(a["dat"]), p(attr), p(nD), *tail)
    else:
        ctf = t(c["ctf"])
        st = lib().thx_insert2d(p(F), p(T), p(O), p(cnt), c["vdim"], c["pf"], p(a["dat"]), p(ctf), *tail)
    assert st == 0, lib().thx_last_error()
    torch.cuda.synchronize()


def host(m):
    F, T, O, cnt = (x.cpu().numpy() for x in m)
    return F.view(np.complex64).reshape(-1), T, O, cnt


def report(tag, r):
    print(f"FIG {tag} insert / budget F.re {r[0]:.3f} F.im {r[1]:.3f} T {r[2]:.3f} O {r[3]:.3f}")


@pytest.mark.parametrize("cid", C.INSERT)
def test_insert2d(cid):
    c, ref = C.get_insert(cid)                       # asserts the tap range
    m = maps(c)
    insert(c, m)
    report(cid, R.check_insert2d(*host(m), ref, P=R.P_HW))
    insert(c, m)                                     # read-modify-write: accumulates onto the first
    report(cid + " twice", R.check_insert2d(*host(m), R.scaled(ref, 2), P=R.P_HW))
    if cid == "ins-cls1":
        z = maps(c)
        insert(c, z, nc=torch.zeros(c["dims"][0], c["dims"][1], dtype=torch.int32, device=DEV))
        R.check_insert2d(*host(z), ref, P=R.P_HW)
        assert np.array_equal(host(z)[3], ref.cnt)


@pytest.mark.parametrize("cid", ["ins-cls", "ins-d-cls"])
def test_insert_i2d(cid):
    """The host adapter, one case per variant: read-modify-write of the
    caller's buffers, called twice."""
    c, ref = C.get_insert(cid)
    nImg, mReco, nPxl = c["dims"]
    nK, size = c["nK"], (c["vdim"] // 2 + 1) * c["vdim"]
    vp = ctypes.c_void_p
    P = lambda a: a.ctypes.data_as(vp)
    hF, hT = np.zeros(2 * nK * size, np.float32), np.zeros(nK * size, np.float32)
    hO, hc = np.zeros(2 * nK), np.zeros(nK, np.int32)
    dat = np.ascontiguousarray(c["dat"]).view(np.float32)
    icp, irp = (np.ascontiguousarray(a * c["pf"], np.int32) for a in (c["iCol"], c["iRow"]))
    rot, tr, off = (np.ascontiguousarray(c[k], np.float64) for k in ("rot", "trans", "off"))
    w, nc = np.ascontiguousarray(c["w"], np.float32), np.ascontiguousarray(c["nc"], np.int32)
    search = c["attr"] is not None
    if search:
        ca = np.ascontiguousarray(np.asarray(c["attr"], np.float32)[:, 1:8])
        nD, pixel, ctf = np.ascontiguousarray(c["nD"], np.float64), float(c["attr"][0, 0]), None
        assert (np.asarray(c["attr"])[:, 0] == c["attr"][0, 0]).all()
    else:
        ctf = np.ascontiguousarray(c["ctf"], np.float32)
    for times in (1, 2):
        st = lib().thx_InsertI2D(P(hF), P(hT), P(hO), P(hc), None, P(dat), P(ctf) if ctf is not None else None, None,
                                 P(w), P(off), P(nc), P(rot), P(tr), P(nD) if search else None,
                                 P(ca) if search else None, P(icp), P(irp), pixel if search else 0.0, int(search),
                                 nK, c["pf"], nPxl, mReco, c["idim"], c["vdim"], nImg)
        assert st == 0, lib().thx_last_error()
        r = R.check_insert2d(hF.view(np.complex64), hT, hO.reshape(nK, 2), hc, R.scaled(ref, times), P=R.P_HW)
        report(f"{cid} InsertI2D x{times}", r)


# --------------------------------------------------------------- global scan
_g2d = {}


def g2d_ref(cid):
    """Class-merged float64 marginals and their per-entry bounds: the scan's
    budget of the adapter's algorithm (4, the default guard) plus what the
    operands carry (scan_input_budget)."""
    if cid not in _g2d:
        c = C.get_g2d(cid)
        nImg, nR, nT, nPxl = c["dims"]
        nK = c["nK"]
        T, _ = PR.phases(c["trans"][None], c["iCol"], c["iRow"], c["idim"])
        rot3, tr3 = np.broadcast_to(c["rot"], (nImg, nR, 2)), np.broadcast_to(c["trans"], (nImg, nT, 2))
        dvps, buds = [], []
        for k in range(nK):
            P = R.project2d_64(c["img"][k], c["rot"], c["iCol"], c["iRow"], c["pf"])      # asserts the tap range
            d64 = SR.dvp64(P, T[0], c["dat"], c["ctf"], c["sig"])
            sm = SR.sums(P, T[0], c["dat"], c["ctf"], c["sig"])
            s2 = R.sums2d(c["img"][k], rot3, tr3, c["dat"], c["ctf"], c["sig"], c["iCol"], c["iRow"], c["idim"],
                          c["pf"])
            dvps.append(d64)
            buds.append(SR.budget(4, 4.0, sm, d64, nPxl) + R.scan_input_budget(s2))
        order = list(range(nK))
        _g2d[cid] = (SR.weights64(dvps, c["pR"], c["pT"], nK, order)[:3],
                     SR.weight_bounds(dvps, buds, c["pR"], c["pT"], nK, order))
    return _g2d[cid]


# the two-worker run ("0,0"): one case, uneven shares (2 + 1 images)
@pytest.mark.parametrize("cid,devices", [(cid, "current") for cid in C.G2D] + [("g2d-69-24-9", "0,0")])
def test_expect_global2d(cid, devices, monkeypatch):
    c = C.get_g2d(cid)
    ref, bounds = g2d_ref(cid)
    nImg, nR, nT, nPxl = c["dims"]
    nK = c["nK"]
    monkeypatch.setenv("THX_DEVICES", devices)
    vp = ctypes.c_void_p
    P = lambda a: a.ctypes.data_as(vp)
    cl = np.ascontiguousarray(c["img"]).view(np.float32)
    dat = np.ascontiguousarray(c["dat"]).view(np.float32)
    ctf, sig = np.ascontiguousarray(c["ctf"]), np.ascontiguousarray(c["sig"])
    rot, tr = np.ascontiguousarray(c["rot"]), np.ascontiguousarray(c["trans"])
    pR, pT = np.ascontiguousarray(c["pR"]), np.ascontiguousarray(c["pT"])
    iCol, iRow = np.ascontiguousarray(c["iCol"], np.int32), np.ascontiguousarray(c["iRow"], np.int32)
    wC, wR, wT = (np.full(n, np.nan, np.float32) for n in (nImg * nK, nImg * nK * nR, nImg * nK * nT))
    st = lib().thx_ExpectGlobal2D(P(cl), P(dat), P(ctf), P(sig), P(tr), P(wC), P(wR), P(wT), P(pR), P(pT), P(rot),
                                  P(iCol), P(iRow), nK, nR, nT, c["pf"], 1, c["idim"], c["vdim"], nPxl, nImg)
    assert st == 0, lib().thx_last_error()
    got = (wC.reshape(nImg, nK), wR.reshape(nImg, nK, nR), wT.reshape(nImg, nK, nT))
    check_marginals(f"{cid} devices {devices}", got, ref, bounds)
