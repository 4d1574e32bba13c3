"""The global scan at its tile edges, against the float64 reference and the
per-sample budget of scan_ref.py, on the cases of
scan_cases.py.  Every case runs through every algorithm that admits it; no
algorithm is the reference for another, except that nT > 160 through algos
2 / 4 must be algo 1's result bit for bit (the same kernel).

Per case and algorithm:
  dvp        algos 2, 4: the dump against dvp64 within budget() at every
             sample; thx_dvp the same with the direct budget;
  baseline   algos 2, 4: exactly the maximum of the dump; algos 0, 1: within
             the image's largest budget of max dvp64;
  marginals  every entry of wR, wT, wC, no share-of-maximum floor: algos 2, 4
             against weights64 of their own dump within 1e-4 of the entry;
             algos 0, 1 against weights64(dvp64) within weight_bounds();
             every entry finite and >= 0;
  workspace  three calls -- the workspace filled with 0xFF bytes and the state
             with 7.0 / 1e30, the workspace zeroed and a fresh state, the
             first again -- give bit-identical outputs, dump included.
"""
import numpy as np
import pytest
import torch

import scan_cases as C
import scan_ref as R
from thunder_amd import ops
from thunder_amd._lib import ThxError, lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALGOS = (0, 1, 2, 4)
Q56 = 2.0 ** -57      # k_scan_mfma adds the wT terms of a block in 2^-56 fixed point

_dev = {}


def up(cid, c):
    if cid not in _dev:
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
        _dev[cid] = dict(rotK=[t(r) for r in c["rotK"]], rotP=t(c["rotP"]), traP=t(c["traP"]),
                         dat=t(c["dat"]), ctf=t(c["ctf"]), sig=t(c["sig"]), pR=t(c["pR"]), pT=t(c["pT"]))
    return _dev[cid]


def stale_state(nImg, nK, nR, nT):
    f = lambda *s, v=7.0: torch.full(s, v, dtype=torch.float32, device=DEV)
    return f(nImg, nK), f(nImg, nK, nR), f(nImg, nK, nT), f(nImg, v=1e30)


def scan(g, c, algo, fill=None, rotP=None, kIdx=0, nK=1, state=None, want_dvp=None):
    """One call; fill: the byte the scan's cached workspace holds on entry.
    -> tuple of numpy arrays (wC, wR, wT, base[, dvp])."""
    nImg, nR, nT, nPxl = c["dims"]
    if fill is not None:
        ops.workspace(lib().thx_global_scan_workspace(nImg, nR, nT, nPxl, algo), DEV).fill_(fill)
    want_dvp = algo >= 2 if want_dvp is None else want_dvp
    kw = dict(guard=c["guard"], want_dvp=True) if want_dvp else {}
    out = ops.global_scan(g["rotP"] if rotP is None else rotP, g["traP"], g["dat"], g["ctf"], g["sig"],
                          g["pR"], g["pT"], kIdx=kIdx, nK=nK, state=state, algo=algo, **kw)
    return out


def host(out):
    return tuple(o.cpu().numpy() for o in out)


def same_bits(a, b):
    return all(x.shape == y.shape and (x.view(np.int32) == y.view(np.int32)).all() for x, y in zip(a, b))


def three_calls(g, c, algo, **kw):
    nImg, nR, nT, _ = c["dims"]
    nK = kw.get("nK", 1)
    a = host(scan(g, c, algo, fill=0xFF, state=stale_state(nImg, nK, nR, nT), **kw))
    b = host(scan(g, c, algo, fill=0, **kw))
    d = host(scan(g, c, algo, fill=0xFF, state=stale_state(nImg, nK, nR, nT), **kw))
    assert same_bits(a, b), "outputs depend on what the workspace or the state held"
    assert same_bits(a, d), "outputs differ between two identical calls"
    return a


def check_marginals(tag, got, ref, bounds, tiny_ok=False):
    """got, ref: (wC, wR, wT); every entry finite, >= 0 and within its bound."""
    worst = {}
    for name, g, r, b in zip(("wC", "wR", "wT"), got, ref, bounds):
        assert np.isfinite(g).all() and (g >= 0).all(), f"{tag} {name}: not finite or negative"
        if tiny_ok and name != "wC":
            top = r.max(axis=-1, keepdims=True)
            tiny = r < 1e-30 * top
            assert (g[tiny] < 2e-30 * np.broadcast_to(top, g.shape)[tiny]).all(), f"{tag} {name}: underflow"
            b = np.where(tiny, np.inf, b)
        worst[name] = R.worst(g, r, b)
    print(f"FIG {tag} marginals / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, f"{tag}: marginal error / bound {worst}"


def check_plain(cid, algo):
    c, d64, sm = C.get(cid)
    nImg, nR, nT, nPxl = c["dims"]
    g = up(cid, c)
    out = three_calls(g, c, algo)
    wC, wR, wT, base = out[:4]
    tag = f"{cid} algo {algo}"
    bud = R.budget(algo, c["guard"] or 4.0, sm, d64, nPxl)
    pR, pT = c["pR"], c["pT"]
    if algo >= 2:
        dump = out[4]
        ratio = R.worst(dump, d64, bud)
        print(f"FIG {tag} dvp / budget {ratio:.3f}")
        assert ratio <= 1.0, f"{tag}: largest dvp error / budget {ratio:.3f}"
        assert (base == dump.max(axis=(1, 2))).all(), f"{tag}: baseline is not the maximum of the dump"
        dd = dump.astype(np.float64)
        ref = R.weights64([dd], pR, pT, 1, [0])
        bounds = [1e-4 * r for r in ref[:3]]
    else:
        btop = bud.max(axis=(1, 2))
        rb = R.worst(base, d64.max(axis=(1, 2)), btop)
        print(f"FIG {tag} baseline / budget {rb:.3f}")
        assert rb <= 1.0, f"{tag}: baseline error / budget {rb:.3f}"
        ref = R.weights64([d64], pR, pT, 1, [0])
        bounds = R.weight_bounds([d64], [bud], pR, pT, 1, [0], quantum=Q56 if algo == 1 else 0.0)
    check_marginals(tag, (wC, wR, wT), ref[:3], bounds, tiny_ok=cid == "underflow")


# ---------------------------------------------------------------------- wide
# first in the file: nT 225 and 256 launch k_scan_mfma<8>, the one
# instantiation whose LDS (67 584 B) is over 64 KiB
@pytest.mark.parametrize("nT", C.WIDE[::-1])
def test_wide(nT):
    cid = f"wide-{nT}"
    c, d64, sm = C.get(cid)
    g = up(cid, c)
    nImg, nR, _, nPxl = c["dims"]
    for algo in (1, 0):
        check_plain(cid, algo)
    one = host(scan(g, c, 1, fill=0xFF))
    for algo in (2, 4):
        assert lib().thx_global_scan_workspace(nImg, nR, nT, nPxl, algo) == \
            lib().thx_global_scan_workspace(nImg, nR, nT, nPxl, 1) > 0
        got = host(scan(g, c, algo, fill=0xFF, want_dvp=False))
        assert same_bits(one, got), f"nT {nT} algo {algo}: not algo 1's result"
        with pytest.raises(ThxError, match=r"status 1\)"):
            scan(g, c, algo, want_dvp=True)


@pytest.mark.parametrize("algo", (1, 2, 4))
def test_nT_257_is_refused(algo):
    c = C.make(3, 5, 257, 17, 657)
    with pytest.raises(ThxError, match=r"status 1\)"):
        scan(up("nT257", c), c, algo, want_dvp=False)


# --------------------------------------------------------------- plain cases
def _plain_params():
    out = []
    for cid, _ in C.plain_cases():
        out += [(cid, a) for a in ALGOS]
    out += [(f"frag_edges-{n}", 0) for n in C.FRAG_EDGES_DIRECT]
    return out


@pytest.mark.parametrize("cid,algo", _plain_params())
def test_case(cid, algo):
    check_plain(cid, algo)


@pytest.mark.parametrize("cid", [cid for cid, _ in C.plain_cases()] +
                         [f"frag_edges-{n}" for n in C.FRAG_EDGES_DIRECT] + [f"wide-{n}" for n in C.WIDE])
def test_thx_dvp(cid):
    c, d64, sm = C.get(cid)
    g = up(cid, c)
    a = ops.dvp(g["rotP"], g["traP"], g["dat"], g["ctf"], g["sig"]).cpu().numpy()
    b = ops.dvp(g["rotP"], g["traP"], g["dat"], g["ctf"], g["sig"]).cpu().numpy()
    assert same_bits((a,), (b,))
    ratio = R.worst(a, d64, R.budget_direct(sm, c["dims"][3]))
    print(f"FIG {cid} thx_dvp dvp / budget {ratio:.3f}")
    assert ratio <= 1.0, f"{cid} thx_dvp: largest dvp error / budget {ratio:.3f}"


# --------------------------------------------------------------------- merge
@pytest.mark.parametrize("algo", ALGOS)
def test_merge(algo):
    """Three classes whose maxima are ordered mid, high, low: 0, 1, 2 (the
    baseline rises, then stays); 0, 2, 1 on a fresh state (stays, then
    rises); then 0 alone on the last run's final state (classes 1, 2 exactly
    0, the baseline class 0's own)."""
    c = C.merge()
    g = up("merge", c)
    nImg, nR, nT, nPxl = c["dims"]
    pR, pT = c["pR"], c["pT"]
    d64, sms, buds = [], [], []
    for k in range(3):
        a = (c["rotK"][k], c["traP"], c["dat"], c["ctf"], c["sig"])
        d64.append(R.dvp64(*a))
        sms.append(R.sums(*a))
        buds.append(R.budget(algo, 4.0, sms[k], d64[k], nPxl))

    def run(order, state):
        dumps = {}
        for k in order:
            out = scan(g, c, algo, fill=0xFF, rotP=g["rotK"][k], kIdx=k, nK=3, state=state)
            state = out[:4]
            if algo >= 2:
                dumps[k] = out[4].cpu().numpy().astype(np.float64)
        return state, dumps

    def check(order, state, dumps):
        wC, wR, wT, base = host(state)
        tag = f"merge {order} algo {algo}"
        if algo >= 2:
            for k, dd in dumps.items():
                assert R.worst(dd, d64[k], buds[k]) <= 1.0, f"{tag}: class {k} dvp over budget"
            dl = [dumps.get(k) for k in range(3)]
            ref = R.weights64(dl, pR, pT, 3, order)
            assert (base == ref[3].astype(np.float32)).all(), f"{tag}: baseline"
            bounds = [1e-4 * r for r in ref[:3]]
        else:
            ref = R.weights64(d64, pR, pT, 3, order)
            bounds = R.weight_bounds(d64, buds, pR, pT, 3, order, quantum=Q56 if algo == 1 else 0.0)
            btop = np.max([b.max(axis=(1, 2)) for b in buds], axis=0)
            assert R.worst(base, ref[3], btop) <= 1.0, f"{tag}: baseline"
        check_marginals(tag, (wC, wR, wT), ref[:3], bounds)

    st, dumps = run((0, 1, 2), stale_state(nImg, 3, nR, nT))
    check((0, 1, 2), st, dumps)
    st, dumps = run((0, 2, 1), None)
    check((0, 2, 1), st, dumps)
    last, dumps = run((0,), st)
    check((0, 2, 1, 0), last, dumps)
    wC, wR, wT, _ = host(last)
    assert (wC[:, 1:] == 0).all() and (wR[:, 1:] == 0).all() and (wT[:, 1:] == 0).all()
    fresh, _ = run((0,), None)
    assert same_bits(host(last), host(fresh)), "kIdx 0 on a used state is not what a fresh state gives"


# ----------------------------------------------------------------- nan_image
@pytest.mark.parametrize("algo", ALGOS)
def test_nan_image(algo):
    """One NaN pixel in image 3: the other 64 images' outputs are bit for bit
    those of the same call with that pixel 0.  Nothing is asserted of image 3."""
    c, z = C.nan_image()
    a = host(scan(up("nan", c), c, algo, fill=0xFF))
    b = host(scan(up("nan0", z), z, algo, fill=0xFF))
    keep = np.arange(c["dims"][0]) != C.NAN_IMG
    assert same_bits([x[keep] for x in a], [x[keep] for x in b])
    assert np.isfinite(b[1]).all()
