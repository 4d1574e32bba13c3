"""The 3D local phase at its tile edges, against the float64 reference and the
per-sample budget of phase_ref.py, on the cases of
phase_cases.py.  Every case runs through every route that admits it; no route
is the reference for another:

  ft         thx_local_phase, half-complex volume, the tile order
  ft-set     the same in set order (pxOrder = NULL)
  cells      volLayout 1, the cell-expanded copy
  ypair      volLayout 2, the y-pair copy
  routed     thx_local_phase_routed without a y-pair copy
  routed-yp  thx_local_phase_routed with one
  ball       thx_local_phase_routed_ball at R = ops.ypair_ball_radius
  d-ft, d-cells   thx_local_phase_d (search cases)

Per case and route:
  workspace  three calls -- the workspace filled with 0xFF bytes and the
             outputs with NaN, the workspace zeroed, the first again -- give
             bit-identical outputs, dump included;
  dvp        every sample of the dump within budget() of dvp64; where one
             workgroup holds an image (fused epilogue) a call without the dump
             gives the same wC, wR, wT, baseL bit for bit;
  baseline   exactly the maximum of the dump;
  marginals  every entry finite, >= 0 and within 1e-4 of itself of weights64
             of the kernel's own dump, no share-of-maximum floor (`underflow`:
             entries below 1e-30 of the row maximum need only be below 2e-30).
"""
import ctypes

import numpy as np
import pytest
import torch

import phase_cases as C
import phase_ref as R
from thunder_amd import ops
from thunder_amd._lib import ThxError, check, lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN_ROUTES = ("ft", "ft-set", "cells", "ypair", "routed", "routed-yp", "ball")
SEARCH_ROUTES = ("d-ft", "d-cells")
RT, TT = 128, 16       # rotations / translations of one workgroup (local.hip)


class Sel(ctypes.Structure):
    _fields_ = [("active", ctypes.c_void_p), ("nActive", ctypes.c_void_p), ("cls", ctypes.c_void_p),
                ("volStride", ctypes.c_longlong)]


class Px:
    """The fields ops.local_phase reads of a pixel set."""

    def __init__(self, c):
        self.n, self.pf, self.idim = len(c["iCol"]), c["pf"], c["idim"]
        self.iCol, self.iRow = c["iCol"], c["iRow"]
        self.order = ops.tile_order(self.iCol, self.iRow)
        self.d_iCol, self.d_iRow, self.d_order = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
                                                  for a in (self.iCol, self.iRow, self.order))


_dev = {}


def up(cid):
    """The device side of a case, built once: the arrays, the pixel set and
    every copy of the volume (per class, stacked)."""
    if cid in _dev:
        return _dev[cid]
    c, _, _ = C.get(cid)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    g = {k: t(c[k]) for k in ("quat", "trans", "dat", "ctf", "sig", "pC", "pR", "pT")}
    if c["nD"]:
        g.update(ctfD=t(c["ctfD"]), pD=t(c["pD"]))
    vols = c["vol"] if c["vol"].ndim == 4 else c["vol"][None]
    g["px"] = px = Px(c)
    g["vol"] = t(vols)
    per = lambda f: torch.stack([f(v) for v in g["vol"]]).contiguous()
    g["cells"], g["ypair"] = per(ops.volume_cells), per(ops.volume_ypair)
    g["ballR"] = Rb = ops.ypair_ball_radius(px)
    g["ball"] = per(lambda v: ops.volume_ypair_ball(v, Rb)) if Rb + 2 <= c["vdim"] // 2 + 1 else None
    g["cls"] = t(c["cls"]) if c["cls"] is not None else None
    _dev[cid] = g
    return g


def routes_of(cid):
    c, _, _ = C.get(cid)
    if c["nD"]:
        return SEARCH_ROUTES
    r2 = int((c["iCol"].astype(np.int64) ** 2 + c["iRow"].astype(np.int64) ** 2).max())
    ball = int(np.ceil(c["pf"] * np.sqrt(r2))) + 2 + 2 <= c["vdim"] // 2 + 1
    return tuple(r for r in PLAIN_ROUTES if r != "ball" or ball)


def phase(cid, route, fill=None, want_dvp=True, active=None, n_active=None, cls="own", vol_stride=None,
          ws_short=0, layout=None):
    """One call through ctypes.  fill: the byte the workspace holds on entry.
    active, n_active: device int tensors or None; cls: "own" = the case's.
    -> (dict of numpy outputs (NaN where nothing was written), route word)."""
    c, _, _ = C.get(cid)
    g = up(cid)
    nImg, nR, nT, nPxl = c["dims"]
    nD, px, p = c["nD"], g["px"], ops._ptr
    search = route.startswith("d-")
    assert search == bool(nD)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    out = dict(wC=nan(nImg), wR=nan(nImg, nR), wT=nan(nImg, nT))
    if search:
        out["wD"] = nan(nImg, nD)
    out["base"] = nan(nImg)
    out["dvp"] = nan(*((nImg, nR, nT, nD) if search else (nImg, nR, nT))) if want_dvp else None
    tiled = route != "ft-set"
    nVisit = len(px.order) if tiled else nPxl
    need = lib().thx_local_phase_workspace(nImg, nR, nT * max(nD, 1), nVisit)
    ws = ops.workspace(need, DEV)
    if fill is not None:
        ws.fill_(fill)
    vs = c["vdim"] * c["vdim"] * (c["vdim"] // 2 + 1)           # float2 elements of one class
    copy, lay, mult = {"ft": ("vol", 0, 1), "ft-set": ("vol", 0, 1), "cells": ("cells", 1, 8), "ypair": ("ypair", 2, 2),
                       "d-ft": ("vol", 0, 1), "d-cells": ("cells", 1, 8)}.get(route, ("vol", 0, 1))
    lay = lay if layout is None else layout
    cls = g["cls"] if isinstance(cls, str) else cls
    sel = None
    if active is not None or n_active is not None or cls is not None:
        sel = Sel(p(active).value if active is not None else None,
                  p(n_active).value if n_active is not None else None,
                  p(cls).value if cls is not None else None,
                  (vs * mult if cls is not None else 0) if vol_stride is None else vol_stride)
    sp = ctypes.addressof(sel) if sel is not None else None
    rword = torch.full((1,), -2, dtype=torch.int32, device=DEV)
    cloud = (p(g["quat"]), nR, p(g["trans"]), nT)
    pri = (p(g["pC"]), p(g["pR"]), p(g["pT"]))
    img = (p(g["dat"]), p(g["ctfD"] if search else g["ctf"]), p(g["sig"]))
    pix = (p(px.d_iCol), p(px.d_iRow), p(px.d_order) if tiled else None, len(px.order), nPxl, px.idim, nImg)
    outs = tuple(p(out[k]) for k in out)
    tail = (p(ws), need - ws_short, ops._stream(DEV))
    vd = (c["vdim"], c["pf"])
    if search:
        fn = "thx_local_phase_d"
        a = (sp, p(g[copy]), lay, *vd, *cloud, nD, *pri, p(g["pD"]), *img, *pix, *outs, *tail)
    elif route in ("routed", "routed-yp"):
        fn = "thx_local_phase_routed"
        a = (sp, p(g["vol"]), p(g["ypair"]) if route == "routed-yp" else None, *vd, *cloud, *pri, *img, *pix,
             *outs, p(rword), *tail)
    elif route == "ball":
        fn = "thx_local_phase_routed_ball"
        a = (sp, p(g["vol"]), p(g["ball"]), g["ballR"], *vd, *cloud, *pri, *img, *pix, *outs, p(rword), *tail)
    elif sel is None:
        fn = "thx_local_phase"
        a = (p(g[copy]), lay, *vd, *cloud, *pri, *img, *pix, *outs, *tail)
    else:
        fn = "thx_local_phase_sel"
        a = (sp, p(g[copy]), lay, *vd, *cloud, *pri, *img, *pix, *outs, *tail)
    check(getattr(lib(), fn)(*a), fn)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}, int(rword.item())


def same_bits(a, b, keys=None):
    keys = list(a if keys is None else keys)
    return all(a[k].shape == b[k].shape and (a[k].view(np.int32) == b[k].view(np.int32)).all() for k in keys)


def three_calls(cid, route, **kw):
    a, ra = phase(cid, route, fill=0xFF, **kw)
    b, rb = phase(cid, route, fill=0, **kw)
    d, rd = phase(cid, route, fill=0xFF, **kw)
    assert same_bits(a, b) and ra == rb, "outputs depend on what the workspace held"
    assert same_bits(a, d) and ra == rd, "outputs differ between two identical calls"
    return a, ra


def check_outputs(cid, route, out, images=None):
    """dvp, baseline and marginals of the images listed (default: all)."""
    c, d64, bud = C.get(cid)
    tag = f"{cid} {route}"
    li = np.arange(len(d64)) if images is None else np.asarray(images)
    dump = out["dvp"][li]
    ratio = R.worst(dump, d64[li], bud[li])
    print(f"FIG {tag} dvp / budget {ratio:.3f}")
    assert ratio <= 1.0, f"{tag}: largest dvp error / budget {ratio:.3f}"
    assert (out["base"][li] == dump.reshape(len(li), -1).max(1)).all(), f"{tag}: baseline is not the dump's maximum"
    pr = [c["pC"][li], c["pR"][li], c["pT"][li]] + ([c["pD"][li]] if c["nD"] else [])
    ref = R.weights64(dump.astype(np.float64), *pr)
    worst = {}
    for name, r in zip(("wC", "wR", "wT", "wD") if c["nD"] else ("wC", "wR", "wT"), ref):
        got = out[name][li]
        assert np.isfinite(got).all() and (got >= 0).all(), f"{tag} {name}: not finite or negative"
        b = 1e-4 * r
        if cid == "underflow" and name != "wC":
            top = np.broadcast_to(r.max(axis=-1, keepdims=True), r.shape)
            tiny = r < 1e-30 * top
            assert (got[tiny] < 2e-30 * top[tiny]).all(), f"{tag} {name}: underflow"
            b = np.where(tiny, np.inf, b)
        worst[name] = R.worst(got, r, b)
    print(f"FIG {tag} marginals / 1e-4 " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, f"{tag}: marginal error / bound {worst}"
    if cid == "priors":
        # a zero prior still gets its own marginal (which does not carry it)
        assert (out["wT"][c["pT"] == 0] > 0).all() and (out["wR"][c["pR"] == 0] > 0).all()


@pytest.mark.parametrize("cid,route", [(cid, r) for cid in C.ALL for r in routes_of(cid)])
def test_case(cid, route):
    c, _, _ = C.get(cid)
    nImg, nR, nT, _ = c["dims"]
    out, rw = three_calls(cid, route)
    check_outputs(cid, route, out)
    if route in ("routed", "routed-yp", "ball"):
        print(f"FIG {cid} {route} route {rw}")
        if c["route"] is not None:
            assert rw == c["route"][route != "routed"], f"{cid} {route}: ran kernel {rw}"
    if not c["nD"] and nR <= RT and nT <= TT:
        bare, _ = phase(cid, route, fill=0xFF, want_dvp=False)
        assert same_bits(out, bare, bare), "the fused epilogue's outputs depend on the dump"


# ----------------------------------------------------------------- selection
SEL_ROUTES = {"route-65": ("ft", "routed", "routed-yp", "ball"), "pix-17": PLAIN_ROUTES,
              "classes": ("ft", "cells", "ypair", "routed-yp", "ball"), "cs-33": SEARCH_ROUTES}


@pytest.mark.parametrize("cid,route", [(c, r) for c, rs in SEL_ROUTES.items() for r in rs])
def test_selection(cid, route):
    """The active list: all images in order; a permutation of a strict subset
    with image 0 and the last image in it, then one without them, the device
    word nActive smaller than the list's allocation (the rest names unlisted
    images).  Listed images equal the unselected run bit for bit, unlisted
    ones keep the NaN every output and the dump were filled with; nActive = 0
    writes nothing.  `classes` runs with cls / volStride throughout, through
    each copy of the volume."""
    c, _, _ = C.get(cid)
    nImg = c["dims"][0]
    ti = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(DEV)
    full, r0 = phase(cid, route, fill=0xFF)
    check_outputs(cid, route, full)
    rng = np.random.default_rng(5)
    mid = rng.permutation(np.arange(1, nImg - 1))
    half = len(mid) // 2
    lists = [np.arange(nImg), rng.permutation(np.r_[0, nImg - 1, mid[:half]]), mid[half:]]
    for lst in lists:
        rest = np.setdiff1d(np.arange(nImg), lst)
        alloc = np.r_[lst, rest] if len(rest) else lst
        out, r1 = phase(cid, route, fill=0xFF, active=ti(alloc), n_active=ti([len(lst)]))
        assert r1 == r0, "the sub-list ran another kernel"
        for k in out:
            assert (out[k][lst].view(np.int32) == full[k][lst].view(np.int32)).all(), f"{k}: listed images differ"
            assert np.isnan(out[k][rest]).all(), f"{k}: an unlisted image was written"
    out, _ = phase(cid, route, fill=0xFF, active=ti(np.arange(nImg)), n_active=ti([0]))
    assert all(np.isnan(v).all() for v in out.values()), "nActive = 0 wrote something"


# ------------------------------------------------------------------ refusals
def test_refusals():
    """Each returns an error before any launch; the next valid call is unaffected."""
    good, _ = phase("pix-17", "ft", fill=0xFF)
    good_d, _ = phase("cs-33", "d-ft", fill=0xFF)
    ti = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(DEV)

    def refused(cid, route, **kw):
        with pytest.raises(ThxError):
            phase(cid, route, fill=0xFF, **kw)
        again, _ = phase(cid, route, fill=0xFF)
        assert same_bits(again, good_d if cid == "cs-33" else good)

    refused("pix-17", "ft", active=ti([0, 1, 2]))                       # active without nActive
    refused("pix-17", "ft", n_active=ti([3]))
    refused("pix-17", "ft", ws_short=1)
    refused("cs-33", "d-ft", layout=2)                                  # a y-pair copy with the search
    refused("pix-17", "ft", cls=ti([0, 0, 0]), vol_stride=0)            # cls with volStride = 0
    # nT * nD = 1025: 205 translations x 5 defocus samples
    c, _, _ = C.get("cs-65")
    g = up("cs-65")
    nImg, nR, _, nPxl = c["dims"]
    nT, nD, px, p = 205, 5, g["px"], ops._ptr
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=DEV)
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    trans, pT = z(nImg, nT, 2), z(nImg, nT)
    outs = [f(nImg), f(nImg, nR), f(nImg, nT), f(nImg, nD), f(nImg), f(nImg, nR, nT, nD)]
    ws = ops.workspace(lib().thx_local_phase_workspace(nImg, nR, nT * nD, len(px.order)), DEV)
    st = lib().thx_local_phase_d(None, p(g["vol"]), 0, c["vdim"], c["pf"], p(g["quat"]), nR, p(trans), nT, nD,
                                 p(g["pC"]), p(g["pR"]), p(pT), p(g["pD"]), p(g["dat"]), p(g["ctfD"]),
                                 p(g["sig"]), p(px.d_iCol), p(px.d_iRow), p(px.d_order), len(px.order), nPxl,
                                 px.idim, nImg, *(p(o) for o in outs), p(ws), ws.numel(), ops._stream(DEV))
    assert st != 0, "nT * nD = 1025 was accepted"
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)
    again, _ = phase("cs-33", "d-ft", fill=0xFF)
    assert same_bits(again, good_d)
