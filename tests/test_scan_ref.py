"""The global scan's float64 reference and per-sample budget, held to account
on the CPU before test_gpu_scan_edges.py holds the kernels to them.

Every figure printed here (pytest -s) is recorded in DESIGN.md section 2.
"""
import numpy as np
import pytest

import scan_cases as C
import scan_ref as R

PLAIN = [cid for cid, _ in C.plain_cases()]
ALL = PLAIN + [f"frag_edges-{n}" for n in C.FRAG_EDGES_DIRECT] + [f"wide-{n}" for n in C.WIDE]


def args(c):
    return c["rotP"], c["traP"], c["dat"], c["ctf"], c["sig"]


def test_emulation_inside_budget():
    """The FP32 sequential sum of each form stays inside its budget on every
    case, and the split products, accumulated in float64, inside eps S_X (of
    the exact products of the same FP32 w) and inside the expanded budget."""
    top = {}
    for cid in ALL:
        c, d, sm = C.get(cid)
        nPxl = c["dims"][3]
        A, B, wr, wi = R.emu_parts32(*args(c))
        xe = R.emu_x_exact64(wr, wi, c["traP"])
        fig = {"direct": R.worst(R.emu_direct32(*args(c)), d, R.budget_direct(sm, nPxl)),
               "expanded": R.worst(R.emu_expanded32(*args(c)), d, R.budget_expanded(sm, nPxl, 1))}
        for algo in (2, 4):
            fig[f"split{algo} X / eps S_X"] = R.worst(R.emu_x_split64(wr, wi, c["traP"], algo), xe,
                                                      R.EPS[algo] * sm["S_X"])
            fig[f"split{algo}"] = R.worst(R.emu_split(*args(c), algo), d, R.budget_expanded(sm, nPxl, algo))
        for k, v in fig.items():
            assert v <= 1.0, (cid, k, v)
            if v > top.get(k, (0, ""))[0]:
                top[k] = (v, cid)
    for k, (v, cid) in top.items():
        print(f"emulation / budget, {k}: largest {v:.3f} at {cid}")


def test_no_reference_marginal_underflows():
    """Outside `underflow`, no reference marginal entry is below 1e-30 of its
    row maximum, so every entry is compared by its bound."""
    for cid in ALL:
        if cid == "underflow":
            continue
        c, d, _ = C.get(cid)
        _, wR, wT, _ = R.weights64([d], c["pR"], c["pT"], 1, [0])
        for w in (wR, wT):
            assert (w >= 1e-30 * w.max(axis=-1, keepdims=True)).all(), cid
    c, d, _ = C.get("underflow")
    _, wR, _, _ = R.weights64([d], c["pR"], c["pT"], 1, [0])
    assert (wR[:, 0, C.UNDERFLOW_R] < 1e-30 * wR.max(axis=-1)[:, 0]).all()
    gap = d.max(axis=(1, 2)) - d[:, C.UNDERFLOW_R].max(axis=-1)
    assert (gap > 200).all(), gap


def test_guard_rounds_fills_the_list():
    """The wave that owns r* has at least 40 samples the guard flags with a
    10 % margin (GCAP = 32): G = |A| + |B| + |X| > 4.4 |dvp| -- and so
    S > 4.4 |dvp|, as S >= G."""
    c, d, sm = C.get("guard_rounds")
    r = int(c["pose"][0][0])
    assert (c["pose"][0] == r).all() and (c["pose"][1] == c["pose"][1][0]).all()
    n = int((sm["G"][:, r] > 4.4 * np.abs(d[:, r])).sum())
    print("guard_rounds: samples of the wave owning r* over 4.4:", n)
    assert n >= 40
    assert int((sm["S"][:, r] > 4.4 * np.abs(d[:, r])).sum()) >= n


def test_rot_blocks_maxima_sit_in_the_last_blocks():
    c, d, _ = C.get("rot_blocks")
    r = d.max(axis=2).argmax(axis=1)
    assert tuple(r) == C.ROT_BLOCKS_POSE and sorted(r // 8) == [256, 257] and (r // 4 >= 512).all()


def test_pad_max_cross_terms_all_negative():
    """A padded column (dvp = A + B) would exceed every real sample of its row."""
    for n in C.PAD_MAX:
        _, d, sm = C.get(f"pad_max-{n}")
        assert (sm["AB"] > d).all(), n


def test_guard_all_flags_every_sample():
    c, d, sm = C.get("guard_all")
    assert (R.guard_form(sm, d, c["guard"]) == 1).all()


def test_guard_band_is_thin():
    """At most 1 % of a guarded case's samples sit where one rounding decides the form."""
    for cid in ALL:
        c, d, sm = C.get(cid)
        frac = float((R.guard_form(sm, d, c["guard"] or 4.0) == 0).mean())
        assert frac <= 0.01, (cid, frac)


def merge_dvps():
    c = C.merge()
    return c, [R.dvp64(c["rotK"][k], c["traP"], c["dat"], c["ctf"], c["sig"]) for k in range(3)]


def test_merge_class_maxima_ordered():
    _, ds = merge_dvps()
    mid, high, low = (d.max(axis=(1, 2)) for d in ds)
    assert (high - mid >= 1).all() and (mid - low >= 1).all(), (mid, high, low)


def test_priors_has_its_zeros():
    c, _, _ = C.get("priors")
    for p in (c["pR"], c["pT"]):
        assert p[0] == 0 and (p == 0).sum() == 2 and abs(p.sum() - 1) < 1e-12
        nz = p[p > 0]
        assert nz.max() / nz.min() > 100


@pytest.mark.parametrize("order", [(0, 1, 2), (0, 2, 1), (0, 1, 2, 0), (0,)])
def test_weights64_against_literal_merge(order):
    c, ds = merge_dvps()
    got = R.weights64(ds, c["pR"], c["pT"], 3, order)
    ref = R.merge_literal(ds, c["pR"], c["pT"], 3, order)
    for g, r in zip(got, ref):
        assert np.allclose(g, r, rtol=1e-12, atol=0), order
    if order[-1] == 0:
        assert (got[0][:, 1:] == 0).all() and (got[1][:, 1:] == 0).all() and (got[2][:, 1:] == 0).all()
        assert (got[3] == ds[0].max(axis=(1, 2))).all()


# ---------------------------------------------------------------- mutations
def dvp_ratio(cid, wrong=None, got=None, algo=4):
    """The GPU test's dvp comparison: got (default: the FP32 emulation of the
    expanded form) against a reference (default: the right one)."""
    c, d, sm = C.get(cid)
    got = R.emu_expanded32(*args(c)) if got is None else got
    return R.worst(got, d if wrong is None else wrong, R.budget_expanded(sm, c["dims"][3], algo))


def test_mutation_last_pixel_dropped():
    for cid in ("chunks-17", "chunks-33"):
        c, d, _ = C.get(cid)
        wrong = R.dvp64(*(a[:, :-1] for a in args(c)))
        assert dvp_ratio(cid) <= 1 < dvp_ratio(cid, wrong), cid


def test_mutation_image_64_is_image_0():
    c, d, _ = C.get("img_tiles-65")
    wrong = d.copy()
    wrong[64] = d[0]
    assert dvp_ratio("img_tiles-65") <= 1 < dvp_ratio("img_tiles-65", wrong)


def test_mutation_translation_column_shifted():
    for cid, t in (("frag_edges-33", 32), ("frag_edges-65", 64), ("frag_edges-160", 159)):
        _, d, _ = C.get(cid)
        wrong = d.copy()
        wrong[:, :, t] = d[:, :, t - 1]
        assert dvp_ratio(cid) <= 1 < dvp_ratio(cid, wrong), cid


def test_mutation_pR_mean_in_wT():
    c, d, sm = C.get("priors")
    bud = R.budget_expanded(sm, c["dims"][3], 4)
    got = R.weights64([R.emu_expanded32(*args(c)).astype(np.float64)], c["pR"], c["pT"], 1, [0])
    _, _, bT = R.weight_bounds([d], [bud], c["pR"], c["pT"], 1, [0])
    ref = R.weights64([d], c["pR"], c["pT"], 1, [0])
    wrong = R.weights64([d], np.full_like(c["pR"], c["pR"].mean()), c["pT"], 1, [0])
    assert R.worst(got[2], ref[2], bT) <= 1 < R.worst(got[2], wrong[2], bT)


SIX = ("hh", "hm", "mh", "hl", "mm", "lh")


def test_mutation_split_products():
    """What the per-sample budget can tell of the algo-4 split, and what it
    cannot.  Dropping hh, hm or mh (>= 2^-9 of a product) is rejected at every
    case by a factor over 100.  Dropping T's lo plane, or one of hl, mm, lh
    (2^-17 .. 2^-18 of a product), moves a sample by about the budget itself
    (measured 0.2 .. 1.3 of it): nPxl u S with nPxl 17 is 2^-19.3 S, and
    S_X is 0.4 S, so one such product is 2^-18.. S before its 17 terms
    partly cancel.  The budget of a whole sample cannot tell these -- not at
    nPxl 17 and SNR 20 either (0.56, 0.85) -- and a smaller S_X / S only
    lowers the figure (`sparse`).  The comparison of the cross term alone,
    against eps S_X, rejects every one of them at every case of more than
    one pixel."""
    extra = C.make(3, 9, 5, 17, 1400, snr=20.0, sign=-1.0)
    # (not pad_max: its T is 1 to within 2^-8, so T's lower pieces carry next to nothing)
    rows = [(cid,) + C.get(cid) for cid in PLAIN if not cid.startswith("pad_max")]
    rows.append(("nPxl 17, SNR 20", extra, R.dvp64(*args(extra)), R.sums(*args(extra))))
    span = {}
    for cid, c, d, sm in rows:
        bud = R.budget_expanded(sm, c["dims"][3], 4)
        A, B, wr, wi = R.emu_parts32(*args(c))
        xe = R.emu_x_exact64(wr, wi, c["traP"])
        muts = {"no lo plane": dict(planes=(0, 1))}
        for i, name in enumerate(SIX):
            muts["no " + name] = dict(kept=tuple(k for j, k in enumerate(R.KEPT[4]) if j != i))
        for name, kw in muts.items():
            whole = R.worst(R.emu_split(*args(c), 4, **kw), d, bud)
            alone = R.worst(R.emu_x_split64(wr, wi, c["traP"], 4, **kw), xe, R.EPS[4] * sm["S_X"])
            lo, hi = span.get(name, (np.inf, 0))
            span[name] = (min(lo, whole), max(hi, whole))
            if name in ("no hh", "no hm", "no mh"):
                assert whole > 100, (cid, name, whole)
            if cid != "one":      # one pixel, one sample: a piece may happen to be 0
                assert alone > 1, (cid, name, alone)
    for name, (lo, hi) in span.items():
        print(f"split mutation '{name}': sample error / budget {lo:.3g} .. {hi:.3g}")
