"""The noise model's float64 restatement (noise_edges_ref.py) and its cases
(noise_cases.py) held to account on the CPU: closed forms, the older
oracle-based reference inside the new budget at P = 1, every case shown to be
the edge its name says, and every named wrong restatement rejected on the case
built for it."""
import copy
from fractions import Fraction

import numpy as np
import pytest

import noise_cases as C
import noise_edges_ref as R
import noise_ref as NR
import twod_ref as T2

DIMS = [False, True]
IDS = ["3d", "2d"]


def _with(c, **kw):
    d = copy.copy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# --------------------------------------------------------------- closed forms
@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
def test_zero_projectee_and_zero_image(two_d):
    c = C.get("grid-pf2", two_d)
    S, _, nrm, _ = R.residual(_with(c, vols=np.zeros_like(c.vols)), 1)
    assert np.array_equal(S[:, 0], S[:, 3]) and not S[:, 2].any()
    px = c.px
    m = R.annulus(px, *c.radii[0])
    assert np.allclose(nrm[0], [R.p2(R.read(a, px))[m].sum() for a in c.img], rtol=1e-14)
    S, _, _, _ = R.residual(_with(c, img=np.zeros_like(c.img)), 1)
    assert np.array_equal(S[:, 0], S[:, 2]) and not S[:, 3].any()


def test_annulus_membership():
    N, r, _, radii = C.SPEC["annulus"]
    px = R.pixels(N, r)
    pts = set(zip(px.iCol.tolist(), px.iRow.tolist()))
    assert set(C.ON_RL2) | set(C.ON_RN2) <= pts
    for (rL, rN) in radii:
        m = R.annulus(px, rL, rN)
        lo, hi = (Fraction(float(np.float32(x))) ** 2 for x in (rL, rN))     # the float's exact square
        brute = np.array([lo <= int(i) ** 2 + int(j) ** 2 < hi for i, j in zip(px.iCol, px.iRow)])
        assert np.array_equal(m, brute)
    m = R.annulus(px, 5.0, 10.0)
    inside = set(zip(px.iCol[m].tolist(), px.iRow[m].tolist()))
    assert set(C.ON_RL2) <= inside and not set(C.ON_RN2) & inside
    assert not R.annulus(px, 7.0, 7.0).any()
    assert R.annulus(px, 0.0, 11.5).all()            # r - 1/2 takes the whole disc
    assert np.float32(np.float64(np.float32(2.3)) ** 2) != np.float64(np.float32(2.3)) ** 2


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
def test_empty_annulus_is_zero(two_d):
    c = C.get("annulus", two_d)
    _, _, nrm, bn = C.ref(c, 1)
    k = c.radii.index((7.0, 7.0))
    assert not nrm[k].any() and not bn[k].any()


# ------------------------------------------------- the old reference, P = 1
@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_reference_within_budget(orc, name, two_d):
    """noise_ref.residual_spectra (slice, CTF and phase from the C oracle in
    FP32) lies within the budget at P = 1"""
    c = C.get(name, two_d)
    S, B, nrm, bn = C.ref(c, 1)
    px = NR.disc(orc, c.N, c.r, c.pf)
    old, oldn = NR.residual_spectra(orc, px, c.r, c.vols, c.vdim, c.pf, c.img, c.ori, c.attr, c.rot,
                                    c.trans, c.off, c.dF, c.cls, c.N, c.radii[0])
    share = [R.worst(old[:, q], S[:, q], B[:, q]) for q in range(4)] + [R.worst(oldn, nrm[0], bn[0])]
    print(f"oracle share {name} {'2d' if two_d else '3d'}: rows " + " ".join(f"{s:.3g}" for s in share[:4])
          + f" norm {share[4]:.3g}")
    assert max(share) <= 1
    ps, bps = R.power_spectrum(c.ori, c.px)
    old_ps = np.stack([NR.power_spectrum(o, px, c.r) for o in c.ori])
    assert R.worst(old_ps, ps, bps) <= 1 and R.worst(S[:, 3], R.power_spectrum(c.img, c.px)[0], bps * 0) == 0


# ---------------------------------------------- every case is what it says
def test_shell_counts():
    counts = {n: R.pixels(*C.SPEC[n][:2]).count for n in C.NAMES}
    assert counts["r1"].tolist() == [1] and counts["r2"].tolist() == [1, 5]
    assert counts["r3"].tolist() == [1, 5, 7]
    big = counts["chunks3"]
    # shells 40, 42, 43, 44, 45 need a third chunk, with a partial tail (41 holds 125 entries)
    assert big[:40].max() <= 128 and big[40:].tolist() == [133, 125, 133, 139, 133, 145]
    for n in C.NAMES:
        N, r, pf, radii = C.SPEC[n]
        assert r <= N // 2 - 1 and r * pf < N * pf // 2 - 1
        assert all(0 <= rL <= rN <= r - 0.5 for rL, rN in radii)
    assert C.SPEC["grid-pf1"][1] == 16 // 2 - 2 and C.SPEC["grid-pf2"][1] == 16 // 2 - 1


def test_table_matches_domain():
    """thx_spectrum_pixels (the host table the kernels walk) lists the brute
    force domain shell by shell in loop order"""
    from thunder_amd import noise
    for n in C.NAMES:
        N, r = C.SPEC[n][:2]
        sp = noise.SpectrumPixels(N, r)
        iCol, iRow, iShell, iPxl, start = NR.by_shell(N, r)
        assert np.array_equal(sp.iCol, iCol) and np.array_equal(sp.iRow, iRow)
        assert np.array_equal(sp.iPxl, iPxl) and np.array_equal(sp.shellStart, start)


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
@pytest.mark.parametrize("name", ["grid-pf2", "grid-pf1"])
def test_grid_cases_sit_on_the_grid(name, two_d):
    c = C.get(name, two_d)
    px = c.px
    assert ((px.iCol == 0) & (px.iRow < 0)).any() and ((px.iCol == 0) & (px.iRow > 0)).any()
    plus = minus = folded_int = wrapped = 0
    for l in range(len(c.rot)):
        xs = R.coords(c, l, px)
        x = xs[0]
        plus += int(((x == 0) & ~np.signbit(x)).sum())
        minus += int(((x == 0) & np.signbit(x)).sum())
        if all((a == np.rint(a)).all() for a in xs):          # weights exactly 0 and 1
            folded_int += int((x < 0).any())
            wrapped += int((np.where(x >= 0, 1.0, -1.0) * xs[1] < 0).any())     # a row below 0 after the fold
    # 2 S S != 1 in FP64: three of the eight 3D rotations carry entries of 2e-16 and
    # so coordinates of that size next to the integers; the others are exact
    assert plus and minus and folded_int >= 2 and wrapped >= 2


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
@pytest.mark.parametrize("name", C.NAMES)
def test_fused_and_unfused_coordinates_agree(name, two_d):
    c = C.get(name, two_d)
    px = c.px
    if two_d:
        assert T2.fused_agree(c.rot, px.iCol, px.iRow, c.pf).all()
        x, y = T2.coords2_64(c.rot, px.iCol, px.iRow, c.pf)
        a, b = T2.cell2(x, y), T2.cell2(x.astype(np.float32), y.astype(np.float32))
        assert np.array_equal(a[0], b[0]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
        assert T2.taps_in_range(x.astype(np.float32), y.astype(np.float32), c.vdim)
    else:
        assert R.fused_agree3(R.mats3(c.rot), px.iCol, px.iRow, c.pf).all()


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
def test_weak_case_is_weak(two_d):
    S, B, _, _ = C.ref(C.get("weak", two_d), 4)
    assert (S[:, 0] < 1e-12 * S[:, 3]).all() and (S[:, 1] < 1e-12 * S[:, 3]).all()
    assert (B[:, 0] < 1e-6 * S[:, 3]).all()          # the budget form stays absolute and small


# ------------------------------------------------ wrong restatements rejected
REJECT = [("mirror0", "grid-pf2"), ("mirror0", "grid-pf1"), ("floor", "r3"), ("le_rN", "annulus"),
          ("gt_rL", "annulus"), ("drop128", "chunks3"), ("noconj", "grid-pf2"), ("noconj", "grid-pf1")]


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
@pytest.mark.parametrize("mut,name", REJECT)
def test_wrong_restatement_rejected(mut, name, two_d):
    c = C.get(name, two_d)
    S, B, nrm, bn = C.ref(c, 4)                      # the wider, device margin
    S2, _, n2, _ = R.residual(c, 4, mut)
    ws = max(R.worst(S2[:, q], S[:, q], B[:, q]) for q in range(4))
    wn = max(R.worst(n2[k], nrm[k], bn[k]) for k in range(len(nrm)))
    print(f"{mut} on {name} {'2d' if two_d else '3d'}: spectra {ws:.3g} norm {wn:.3g} of the budget")
    if mut in ("le_rN", "gt_rL"):
        assert wn > 1 and ws == 0
        k = c.radii.index((5.0, 10.0))
        assert R.worst(n2[k], nrm[k], bn[k]) > 1
    else:
        assert ws > 1
    if mut in ("mirror0", "drop128", "floor"):
        ps, bps = R.power_spectrum(c.ori, c.px)
        assert R.worst(R.power_spectrum(c.ori, R.pixels(c.N, c.r, mut), mut)[0], ps, bps) > 1


@pytest.mark.parametrize("n_group,r", C.ACC_SHAPE)
@pytest.mark.parametrize("n", C.ACC_N)
def test_accumulate_restatements(n, n_group, r):
    """the batched walk equals noise_ref.sigma_sums bit for bit; the wrong
    walks do not"""
    a = C.acc_case(n, n_group, r)
    for spectra in (a.spectra, a.nan):
        for group in (a.group, None):
            assert R.same_bits(R.accumulate_emu(spectra, group, n_group), R.sigma_sums(spectra, group, n_group))
    good = R.sigma_sums(a.spectra, a.group, n_group)
    assert np.isfinite(good).all()
    if n_group >= 3:
        assert not good[:, 1].any() and good[0, -1, r] == 1        # an empty group, the last image alone
    assert not R.same_bits(R.accumulate_emu(a.spectra, a.group, n_group, mut="last_twice"), good) or n % 8 == 0
    assert not R.same_bits(R.accumulate_emu(a.spectra, a.group, n_group, mut="skip8"), good) or n <= 8
    # the NaN stays in its own group's row-2 entry
    bad = R.sigma_sums(a.nan, a.group, n_group)
    l, u = a.at
    where = np.zeros_like(bad, bool)
    where[2, a.group[l], u] = True
    if n > 2 and r > 1:
        assert np.isposinf(bad[2, a.group[0], r - 1])
        where[2, a.group[0], r - 1] = True
    assert np.isnan(bad[2, a.group[l], u]) and np.isfinite(bad[~where]).all()
    assert R.same_bits(bad[~where], good[~where])
    leak = R.accumulate_emu(a.nan, a.group, n_group, mut="mulzero")
    assert np.isnan(leak[2, :, u]).all() and (n_group == 1 or not R.same_bits(leak, bad))


@pytest.mark.parametrize("a,b", C.ACC_SPLIT)
def test_accumulate_split_restated(a, b):
    for n_group, r in C.ACC_SHAPE:
        c = C.acc_case(a + b, n_group, r)
        one = R.accumulate_emu(c.spectra, c.group, n_group)
        two = R.accumulate_emu(c.spectra[a:], c.group[a:], n_group,
                               acc=R.accumulate_emu(c.spectra[:a], c.group[:a], n_group))
        assert R.same_bits(one, two)


@pytest.mark.parametrize("n", C.ROWS_N)
def test_rows_restatement(n):
    c = C.rows_case(n)
    for group in (c.group, None):
        out = R.rows_emu(c.rcp, group, c.iSig, 5)
        assert not (out == R.SENTINEL).any()
        bad_u = (c.iSig < 0) | (c.iSig >= c.n_col)
        for l in range(5):
            g = 0 if group is None else group[l]
            if 0 <= g < c.n_group:
                assert np.isnan(out[l, bad_u]).all()
                assert np.array_equal(out[l, ~bad_u], c.rcp[g, c.iSig[~bad_u]].astype(np.float32))
            else:
                assert np.isnan(out[l]).all()
        assert R.same_bits(R.rows_emu(c.rcp, group, c.iSig, 5, mut="one_trip"), out) == (n <= R.ROWS_SPAN)


@pytest.mark.parametrize("N", C.SCALE_N)
def test_scale_restatement(N):
    c = C.scale_case(N)
    per = N * (N // 2 + 1)
    assert (per <= R.SCALE_SPAN) == (N == 180) and -(-per // 256) >= 64
    for s in C.SCALE:
        out = R.scale_emu(c.img[1:4], s)
        assert np.array_equal(out, c.img[1:4] * s[:, None, None])
        assert R.same_bits(R.scale_emu(c.img[1:4], s, mut="one_trip"), out) == (N == 180)
