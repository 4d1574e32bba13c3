"""CPU check of the local phase's float64 reference, its budget and its cases
(phase_ref.py, phase_cases.py; DESIGN.md section 2 quotes the figures printed
here).  No GPU, no oracle: the reference is checked against a second, literal
restatement, the budget against an FP32 emulation of the kernel's sums, the
cases against the conditions the device test relies on, and the comparison
against wrong restatements it has to reject."""
import numpy as np
import pytest

import phase_cases as C
import phase_ref as R


# ----------------------------------------------------------------- emulation
@pytest.mark.parametrize("cid", C.ALL)
def test_emulation_stays_inside_the_budget(cid):
    c, d64, bud = C.get(cid)
    ratio = R.worst(R.emu32(*C.args(c)), d64, bud)
    print(f"FIG {cid} emu32 / budget {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------- reference, literally
@pytest.mark.parametrize("cid", ["pix-17", "fold", "wrap", "wide", "ball-edge"])
def test_project64_against_the_full_hermitian_cube(cid):
    c, _, _ = C.get(cid)
    v = c["vol"].astype(np.complex128)
    vd = c["vdim"]
    m = np.mod(-np.arange(vd), vd)
    assert (v[:, :, 0] == np.conj(v[m][:, m][:, :, 0])).all(), "x = 0 plane not Hermitian"
    a = R.project64(c["vol"], c["quat"], c["iCol"], c["iRow"], c["pf"])
    b = R.project_full(c["vol"], c["quat"], c["iCol"], c["iRow"], c["pf"])
    err = np.abs(a - b).max() / np.abs(a).max()
    print(f"FIG {cid} project64 vs full cube {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("cid", ["priors", "ties", "underflow", "cs-33"])
def test_weights64_against_the_literal_loop(cid):
    c, d64, _ = C.get(cid)
    pr = (c["pC"], c["pR"], c["pT"]) + ((c["pD"],) if c["nD"] else ())
    for a, b in zip(R.weights64(d64, *pr), R.weights_literal(d64, *pr)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- conditions
def _coords(c):
    return R.coords64(c["quat"], c["iCol"], c["iRow"], c["pf"])


@pytest.mark.parametrize("cid", C.ALL)
def test_case_conditions(cid):
    c, d64, bud = C.get(cid)
    x, y, z = _coords(c)
    assert not ((np.abs(x) > 0) & (np.abs(x) < 1e-4)).any(), "a fold FP32 and FP64 may decide apart"
    for a in (x, y, z):
        n = np.rint(a)
        assert not ((np.abs(a - n) < 1e-4) & (a != n)).any(), "a floor FP32 and FP64 may decide apart"
        assert (a.astype(np.float32)[a == n] == n[a == n]).all()
    assert np.isfinite(d64).all() and (bud > 0).all()
    pr = (c["pC"], c["pR"], c["pT"]) + ((c["pD"],) if c["nD"] else ())
    ws = R.weights64(d64, *pr)
    if cid != "underflow":
        span = d64.reshape(len(d64), -1)
        assert (span.max(1) - span.min(1)).max() < 60
        for w, p in zip(ws[1:-1], pr[1:]):
            live = p > 0
            assert (w[live] >= 1e-30 * w.max(axis=-1, keepdims=True).repeat(w.shape[-1], -1)[live]).all()


def test_conditions_of_the_named_cases():
    c, d64, bud = C.get("priors")
    assert ((c["pR"] == 0).sum(1) == 2).all() and ((c["pT"] == 0).sum(1) == 2).all() and (c["pC"] != 1).all()

    c, d64, _ = C.get("ties")
    for l in range(3):
        r = c["pose"][0][l]
        assert (c["quat"][l, r] == c["quat"][l, (r + 1) % 9]).all()
        assert (d64[l, r] == d64[l, (r + 1) % 9]).all() and d64[l, r].max() == d64[l].max()

    c, d64, _ = C.get("underflow")
    span = d64.reshape(3, -1)
    assert ((span.max(1) - span.min(1)) > 200).all()
    w = R.weights64(d64, c["pC"], c["pR"], c["pT"])
    assert (w[1] < 1e-30 * w[1].max(1, keepdims=True)).any()

    c, d64, bud = C.get("classes")
    assert set(c["cls"]) == {0, 1}
    other = R.dvp64(*C.args(c)[:-1], 1 - c["cls"])
    gap = (np.abs(other - d64) / bud).min()
    print(f"FIG classes smallest class gap / budget {gap:.1f}")
    assert gap >= 10

    c, _, _ = C.get("wrap")
    h = c["vdim"] // 2
    _, (x0, y0, z0), _ = R.cell(*_coords(c))
    faces = {"y0 + 1 = vdim/2": (y0 + 1 == h), "z0 + 1 = vdim/2": (z0 + 1 == h), "x0 = vdim/2 - 1": (x0 == h - 1),
             "y0 = -vdim/2": (y0 == -h), "z0 = -vdim/2": (z0 == -h), "y0 = -1": (y0 == -1), "z0 = -1": (z0 == -1)}
    print("FIG wrap samples per face " + ", ".join(f"{k}: {int(v.sum())}" for k, v in faces.items()))
    assert all(v.any() for v in faces.values())

    c, _, _ = C.get("ball-edge")
    r2 = int((c["iCol"].astype(np.int64) ** 2 + c["iRow"].astype(np.int64) ** 2).max())
    Rb = int(np.ceil(c["pf"] * np.sqrt(r2))) + 2        # ops.ypair_ball_radius
    _, (x0, y0, z0), _ = R.cell(*_coords(c))
    for name, a in (("x", x0), ("y", y0), ("z", z0)):
        edge = np.maximum(a, -a - 1) >= Rb - 3
        print(f"FIG ball-edge R {Rb}: samples with floor |{name}| >= R - 3: {int(edge.sum())}")
        assert edge.any()
    assert ((z0 + Rb) % 2 == 0).any() and ((z0 + Rb) % 2 == 1).any()

    c, _, _ = C.get("fold")
    x, y, z = (a.astype(np.float32) for a in _coords(c))
    zero = x == 0
    assert (zero & ~np.signbit(x)).any() and (zero & np.signbit(x)).any(), "needs x = +0.0 and -0.0"
    assert ((x > -1) & (x < 0)).any() and ((x > 0) & (x < 1)).any(), "no cell straddles x = 0"
    for a in _coords(c):
        assert (a[:, :4] == np.rint(a[:, :4])).all()


# ----------------------------------------------------------------- mutations
def _factor(tag, mut, d64, bud, where=None):
    err = np.abs(mut - d64) / bud
    f = float(err.max() if where is None else err[where].max())
    print(f"FIG mutation {tag}: error / budget {f:.3g}")
    return f


def _sub(c, keep):
    k = dict(c)
    for n in ("dat", "ctf", "sig", "iCol", "iRow"):
        k[n] = c[n][..., keep]
    return k


def test_the_budget_rejects_wrong_restatements():
    for cid in ("pix-17", "pix-33"):
        c, d64, bud = C.get(cid)
        n = c["dims"][3]
        assert _factor(f"last pixel dropped ({cid})", R.dvp64(*C.args(_sub(c, np.arange(n - 1)))), d64, bud) > 1

    # a padding entry counted: pixel (0, 0) -- the DC voxel -- with pixel 0's data
    c, d64, bud = C.get("pix-17")
    k = _sub(c, np.r_[np.arange(17), 0])
    k["iCol"], k["iRow"] = np.r_[c["iCol"], 0].astype(np.int32), np.r_[c["iRow"], 0].astype(np.int32)
    assert _factor("padding entry counted as pixel (0, 0) (pix-17)", R.dvp64(*C.args(k)), d64, bud) > 1

    # tap 0 of (image 0, rotation 2, pixel 5) read from the next cell in x
    P = R.project64(c["vol"], c["quat"], c["iCol"], c["iRow"], c["pf"], mut=("tap", 2 * 17 + 5))
    assert (P[1:] == c["P"][1:]).all() and (P[0, 2, 5] != c["P"][0, 2, 5])
    assert _factor("one tap from the neighbouring cell (pix-17)", R.dvp64(*C.args(c), P=P), d64, bud,
                   where=(0, 2)) > 1

    c, d64, bud = C.get("fold")
    P = R.project64(c["vol"], c["quat"], c["iCol"], c["iRow"], c["pf"], mut="noconj")
    assert _factor("conjugate of folded samples omitted (fold)", R.dvp64(*C.args(c), P=P), d64, bud) > 1

    c, d64, bud = C.get("wrap")
    P = R.project64(c["vol"], c["quat"], c["iCol"], c["iRow"], c["pf"], mut="nowrap")
    assert _factor("no wrap of y0 + 1 (wrap)", R.dvp64(*C.args(c), P=P), d64, bud) > 1

    c, d64, bud = C.get("rot-129")
    m = d64.copy()
    m[:, 128] = d64[:, 0]
    assert _factor("rotation 128 taken for rotation 0 (rot-129)", m, d64, bud, where=(slice(None), 128)) > 1

    c, d64, bud = C.get("tr-17x3")
    m = d64.copy()
    m[:, :, 16] = d64[:, :, 15]
    assert _factor("translation column 16 taken for 15 (tr-17x3)", m, d64, bud,
                   where=(slice(None), slice(None), 16)) > 1

    c, d64, bud = C.get("cs-33")
    k = dict(c, ctfD=np.roll(c["ctfD"], 1, axis=1))
    assert _factor("CTF row off by one (cs-33)", R.dvp64(*C.args(k)), d64, bud) > 1

    c, d64, bud = C.get("classes")
    m = R.dvp64(*C.args(c)[:-1], np.zeros_like(c["cls"]))
    one = c["cls"] == 1
    assert (m[~one] == d64[~one]).all()
    assert _factor("class 0's volume for a class-1 image (classes)", m, d64, bud, where=one) > 1

    # marginals: the bar is 1e-4 of every entry of weights64 of the same dvp
    c, d64, bud = C.get("priors")
    wC, wR, wT, _ = R.weights64(d64, c["pC"], c["pR"], c["pT"])
    flat = np.broadcast_to(c["pR"].mean(1, keepdims=True), c["pR"].shape)
    bad = R.weights64(d64, c["pC"], flat, c["pT"])[2]
    f = float((np.abs(bad - wT) / (1e-4 * wT)).max())
    print(f"FIG mutation pR mean used in wT (priors): error / bound {f:.3g}")
    assert f > 1
