"""The oracle's insert and gather against the float64 reference of
scatter_ref.py, per voxel, at the phase margin P = 1 -- the budget is validated
here against the reference restatement, never against a kernel -- and the
power of that per-voxel check against the suite's older ``1e-5 max|ref|`` one.

Largest err / budget of the oracle (F.re, F.im, T) per case of
insert_cases.py:

    edge pf 2 rU 7   0.36 0.35 0.15      edge pf 2 rU 6   0.25 0.28 0.17
    edge pf 1 rU 6   0.16 0.23 0.13      edge pf 1 rU 5   0.07 0.11 0.09
    chunks           0.04 0.06 0.15      grouping         0.02 0.05 0.24
    many tiles       0.48 0.47 0.21      tiled paths      0.50 0.56 0.24
    CTF search: edge pf 1 rU 5  0.14 0.15 0.14   chunks (40)  0.17 0.21 0.24
    gather: 0.05 (pf 1 rU 6), 0.06 (pf 2 rU 7)

so the oracle's own FP32 rounding takes up to 0.56 of the budget the
device is then held to (with its phase term four times wider)."""
import numpy as np
import pytest

import insert_cases as ic
import scatter_ref as sr

CASES = {
    "edge_pf2_r7": lambda o: ic.edge(o, 2, 7),
    "edge_pf2_r6": lambda o: ic.edge(o, 2, 6),
    "edge_pf1_r6": lambda o: ic.edge(o, 1, 6),
    "edge_pf1_r5": lambda o: ic.edge(o, 1, 5),
    "chunks": ic.chunks,
    "grouping": ic.grouping,
    "many": ic.many,
    "tiled_paths": ic.tiled_paths,
}


def _ref(c, **kw):
    return sr.insert_f64(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"], c["w"],
                         c["px"], c["N"], **kw)


def _orc(orc, c):
    return orc.insert_batch(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"],
                            c["w"], c["px"], c["N"])


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_insert_within_budget(orc, name):
    c = CASES[name](orc)
    ref = _ref(c)
    F, T, O, cnt = _orc(orc, c)
    r = sr.check_insert(F, T, ref, P=1)
    print(f"{name}: oracle err / budget F.re {r[0]:.2f} F.im {r[1]:.2f} T {r[2]:.2f}")
    assert np.allclose(O, ref.O, rtol=1e-12, atol=1e-12) and cnt == ref.cnt


@pytest.mark.parametrize("name", ["edge_pf1_r5", "chunks40"])
def test_oracle_ctf_search_insert_within_budget(orc, name):
    c = ic.chunks(orc, mReco=40) if name == "chunks40" else CASES[name](orc)
    attr, nD = ic.ctf_search_inputs(c, 500)
    ref = _ref(dict(c, ctf=None), attr=attr, nD=nD)
    F, T, O, cnt = orc.insert_batch_d(c["vdim"], c["pf"], c["dat"], attr, nD, c["quat"], c["trans"],
                                      c["off"], c["w"], c["px"], c["N"])
    r = sr.check_insert(F, T, ref, P=1)
    print(f"{name}: oracle err / budget F.re {r[0]:.2f} F.im {r[1]:.2f} T {r[2]:.2f}")
    assert np.allclose(O, ref.O, rtol=1e-12, atol=1e-12) and cnt == ref.cnt


def _volume(vdim, seed):
    rng = np.random.default_rng(seed)
    shape = (vdim, vdim, vdim // 2 + 1)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("name", ["edge_pf1_r6", "edge_pf2_r7"])
def test_oracle_gather_within_budget(orc, name):
    c = CASES[name](orc)
    vol = _volume(c["vdim"], 9)
    mats = sr._mats(c["quat"][0])
    P, b = sr.project_f64(vol, c["vdim"], c["pf"], mats, c["px"])
    got = np.stack([orc.project3d(vol, c["vdim"], c["pf"], m, c["px"]) for m in mats])
    r = max(sr.worst(got.real, P.real, b), sr.worst(got.imag, P.imag, b))
    print(f"{name}: oracle gather err / budget {r:.2f}")
    assert r <= 1


def test_edge_case_coordinates_sit_on_the_grid_and_just_below_zero(orc):
    """What the edge cases are for: on-grid rotations put coordinates exactly
    on integers (zero-weight taps) and, through sqrt(1/2)'s rounding, a few
    units of 1e-16 below zero (a fold decided by the last bit); the largest
    radius the front end admits (rU pf < vdim / 2 - 1) puts taps on column
    pf (rU - 1) + 1, the outermost any insert reaches in this box."""
    c = ic.edge(orc, 2, 7)
    x, y, z = sr.coords_f32(sr._mats(c["quat"][0][:8]), c["px"].iCol, c["px"].iRow, c["pf"])
    allc = np.concatenate([a.reshape(-1) for a in (x, y, z)])
    assert np.sum(allc == np.floor(allc)) > 100
    assert np.sum((x > -1e-6) & (x < 0)) > 0
    t = sr.image_taps(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"], c["w"],
                      c["px"], c["N"], 0, 16)
    assert (t["idx"] % (c["vdim"] // 2 + 1)).max() == c["pf"] * (c["rU"] - 1) + 1


# ------------------------------------------------------------ checker power
def _old_check(gF, gT, F, T):
    return (np.max(np.abs(gF - F)) <= 1e-5 * np.max(np.abs(F)) and
            np.max(np.abs(gT - T)) <= 1e-5 * np.max(np.abs(T)))


def _new_check(gF, gT, ref):
    try:
        sr.check_insert(gF, gT, ref, P=1)
    except AssertionError:
        return False
    return True


@pytest.fixture(scope="module")
def power(orc):
    c = ic.edge(orc, 2, 6)
    ref = _ref(c)
    F, T, _, _ = _orc(orc, c)
    t = sr.image_taps(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"], c["w"],
                      c["px"], c["N"], 0, 16)
    assert _new_check(F, T, ref) and _old_check(F, T, F, T)
    return c, ref, F, T, t


def test_check_rejects_a_misplaced_tap(power):
    """One tap of one pixel (a median-|ctf| one) lands on the neighbouring column."""
    c, ref, F, T, t = power
    m = 9                                       # a uniform rotation
    p = int(np.argsort(np.abs(c["ctf"][0]))[c["px"].n // 2])
    k = int(np.argmax(t["wt"][:, m, p]) & ~1)   # an i = 0 tap: its +1 column stays inside the row
    v = t["idx"][k, m, p]
    gF = F.copy()
    gF[v] -= np.complex64(t["val"][m, p] * t["wt"][k, m, p])
    gF[v + 1] += np.complex64(t["val"][m, p] * t["wt"][k, m, p])
    assert not _new_check(gF, T, ref)


def test_check_rejects_a_dropped_halo_tap(power):
    """An entry whose cell corner is the last of a 16-corner tile (row
    y0 + R = 15 mod 16) loses its +1 taps in y, the next tile's halo."""
    c, ref, F, T, t = power
    R = c["pf"] * c["rU"] + 2
    y0 = t["corner"][1]
    on_edge = ((y0 + R) % 16 == 15)
    on_edge[:8] = False                          # the on-grid rotations' +1 taps weigh 0
    assert on_edge.any()
    wj = t["wt"][2] + t["wt"][3] + t["wt"][6] + t["wt"][7]
    m, p = np.unravel_index(np.argmax(np.where(on_edge, wj * np.abs(t["val"]), 0)), y0.shape)
    gF, gT = F.copy(), T.copy()
    for k in (2, 3, 6, 7):
        gF[t["idx"][k, m, p]] -= np.complex64(t["val"][m, p] * t["wt"][k, m, p])
        gT[t["idx"][k, m, p]] -= np.float32(t["tv"][m, p] * t["wt"][k, m, p])
    assert not _new_check(gF, gT, ref)


def test_check_rejects_a_missing_conjugation_on_the_fold(power):
    """A folded sample in the x = 0 cell (columns 0 and 1) inserted unconjugated."""
    c, ref, F, T, t = power
    cand = t["conj"] & (t["corner"][0] == 0)
    assert cand.any()
    m, p = np.unravel_index(np.argmax(np.where(cand, np.abs(t["val"].imag), 0)), cand.shape)
    gF = F.copy()
    for k in range(8):
        gF[t["idx"][k, m, p]] += np.complex64((np.conj(t["val"][m, p]) - t["val"][m, p]) * t["wt"][k, m, p])
    assert not _new_check(gF, T, ref)


def test_check_rejects_a_weak_t_tap_the_global_bound_accepts(orc, power):
    """One tap's T scaled by 1 + 1e-3 at a voxel whose T is below 1e-3 of the
    largest: the change is below 1e-6 max T, a tenth of what the global bound
    allows, and above the voxel's budget -- the gap the per-voxel check closes."""
    c, ref, F, T, _ = power
    weak = ref.support & (ref.T < 1e-3 * ref.T.max())
    assert weak.any()
    best = None
    for l in range(len(c["dat"])):
        t = sr.image_taps(c["vdim"], c["pf"], c["dat"], c["ctf"], c["quat"], c["trans"], c["off"],
                          c["w"], c["px"], c["N"], l, 16)
        gain = np.where(weak[t["idx"]], t["tv"][None] * t["wt"] / ref.bT()[t["idx"]], 0)
        k, m, p = np.unravel_index(np.argmax(gain), gain.shape)
        if best is None or gain[k, m, p] > best[0]:
            best = (gain[k, m, p], t["idx"][k, m, p], t["tv"][m, p] * t["wt"][k, m, p])
    _, v, tap = best
    gT = T.copy()
    gT[v] += np.float32(1e-3 * tap)
    assert gT[v] != T[v]
    assert not _new_check(F, gT, ref)
    assert _old_check(F, gT, F, T)


# ---------------------------------------------------------------- adjoint
def test_reference_insert_is_the_adjoint_of_the_reference_gather(orc):
    """Re sum_i conj(project(V)_i) d_i = Re sum_v conj(V_v) insert(d)_v in
    float64 (unit CTF and weight, zero shift): the identity holds tap by tap."""
    c = ic.edge(orc, 2, 7)
    nImg, mReco = c["quat"].shape[:2]
    vol = _volume(c["vdim"], 11)
    one = dict(c, ctf=np.ones_like(c["ctf"]), trans=np.zeros_like(c["trans"]),
               off=np.zeros_like(c["off"]), w=np.ones(nImg, np.float32))
    ref = _ref(one)
    lhs = 0.0
    for l in range(nImg):
        P, _ = sr.project_f64(vol, c["vdim"], c["pf"], sr._mats(c["quat"][l]), c["px"])
        lhs += np.sum(np.conj(P) * c["dat"][l].astype(np.complex128)[None, :]).real
    rhs = np.sum(np.conj(vol.astype(np.complex128).reshape(-1)) * ref.F).real
    assert abs(lhs - rhs) <= 1e-12 * abs(rhs) and abs(rhs) > 1
