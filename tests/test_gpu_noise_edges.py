"""The noise-model kernels (csrc/noise.hip) at their edges, against the float64
restatement and the counted absolute budgets of noise_edges_ref.py (DESIGN.md
section 2) on the cases of noise_cases.py, through thunder_amd.noise.

  k_residual / k_power_spectrum / k_init_ps   err / budget <= 1 per (image,
      row, shell) and per norm at the device's phase margin P = 4; two calls
      bit-identical; the sums of initSigma bit-equal to FP64 in-order sums of
      the device's own terms
  k_sigma_accumulate   rows 0, 1 and the counts bit-equal to
      noise_ref.sigma_sums, row 2 within (n + 2) 2^-53 sum |t|, a NaN / inf
      term only in its own group's entry, split calls bit-equal to one call
  k_sig_rcp_rows, k_img_scale   exact, past the grid caps; guard images
      bit-identical
  nImg = 0 leaves every output untouched."""
import types

import numpy as np
import pytest
import torch

import noise_cases as C
import noise_edges_ref as R
from thunder_amd import noise, ops
from thunder_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P_DEV = 4
DIMS = [False, True]
IDS = ["3d", "2d"]


def T_(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


_dev = {}


def up(name, two_d):
    key = (name, two_d)
    if key not in _dev:
        c = C.get(name, two_d)
        g = types.SimpleNamespace(**{k: T_(getattr(c, k)) for k in ("vols", "img", "ori", "attr", "rot", "trans",
                                                                     "off", "dF", "cls")})
        g.sp = noise.SpectrumPixels(c.N, c.r, DEV)
        g.stack = types.SimpleNamespace(N=c.N, imgFT=g.img, oriFT=g.ori, attr=g.attr, r_mask=0.35 * c.N)
        _dev[key] = g
    return _dev[key]


def spectra_of(c, g, radii):
    return noise.residual_spectra(g.vols, g.img, g.ori, g.attr, g.rot, g.trans, g.sp, c.pf, g.off, g.dF, g.cls,
                                  norm_radii=radii)


@pytest.mark.parametrize("two_d", DIMS, ids=IDS)
@pytest.mark.parametrize("name", C.NAMES)
def test_residual_spectra_and_norms(name, two_d):
    c, g = C.get(name, two_d), up(name, two_d)
    S, B, nrm, bn = C.ref(c, P_DEV)
    tag = f"{name} {'2d' if two_d else '3d'}"
    first = None
    for k, radii in enumerate(c.radii):
        got, norm = spectra_of(c, g, radii)
        again, norm2 = spectra_of(c, g, radii)
        assert torch.equal(got, again) and torch.equal(norm, norm2), f"{tag}: two calls differ"
        first = got if first is None else first
        assert torch.equal(got, first), f"{tag}: the spectra depend on the norm radii"
        wn = R.worst(norm.cpu().numpy(), nrm[k], bn[k])
        print(f"norm {tag} radii {radii}: err / budget {wn:.3g}")
        assert wn <= 1
    got = first.cpu().numpy()
    rows = [R.worst(got[:, q], S[:, q], B[:, q]) for q in range(4)]
    print(f"residual {tag}: err / budget rows " + " ".join(f"{w:.3g}" for w in rows))
    assert max(rows) <= 1
    # the same kernel through the noise model: norms (no oriFT, no offset) and update
    nm = noise.NoiseModel(c.N, 2, DEV, r=c.r, n_col=c.N // 2)
    rL, rN = c.radii[0]
    norm = nm.norms(g.stack, g.vols, g.rot, g.trans, rL, rN, c.pf, g.dF, g.cls)
    assert torch.equal(norm, spectra_of(c, g, c.radii[0])[1])
    group = T_((np.arange(len(c.img)) % 2).astype(np.int32))
    nm.update(g.stack, g.vols, g.rot, g.trans, c.pf, g.off, g.dF, g.cls, group)
    assert torch.equal(nm.spectra, first)
    assert R.same_bits(nm.acc.cpu().numpy()[:2], R.sigma_sums(got, group.cpu().numpy(), 2)[:2])


@pytest.mark.parametrize("name", C.NAMES)
def test_power_spectrum_and_init(name):
    c, g = C.get(name, False), up(name, False)
    ref, bud = R.power_spectrum(c.ori, c.px)
    ps = noise.power_spectrum(g.ori, g.sp)
    assert torch.equal(ps, noise.power_spectrum(g.ori, g.sp))
    w = R.worst(ps.cpu().numpy(), ref, bud)
    print(f"power spectrum {name}: err / budget {w:.3g}")
    assert w <= 1
    # initSigma's sums: FP64, image order, of the same shell_power terms / of every stored float
    want_ps = torch.zeros(c.r, dtype=torch.float64, device=DEV)
    want_avg = torch.zeros(c.N, c.N // 2 + 1, 2, dtype=torch.float64, device=DEV)
    for l in range(len(c.ori)):
        want_ps = want_ps + ps[l].double()
        want_avg = want_avg + torch.view_as_real(g.ori[l]).double()
    avg, pss = noise.sigma_init_accumulate(g.ori, g.sp)
    assert torch.equal(pss, want_ps) and torch.equal(avg, want_avg)
    a, p = noise.sigma_init_accumulate(g.ori[:1].contiguous(), g.sp)
    a, p = noise.sigma_init_accumulate(g.ori[1:].contiguous(), g.sp, a, p)
    assert torch.equal(p, want_ps) and torch.equal(a, want_avg)
    nm = noise.NoiseModel(c.N, 2, DEV, r=c.r, n_col=c.N // 2)
    nm.init_from(g.stack)
    assert torch.equal(nm.ps_sum, want_ps) and torch.equal(nm.avg_sum, want_avg)


def check_acc(got, spectra, group, n_group, tag):
    got = got.cpu().numpy()
    ref = R.sigma_sums(spectra, group, n_group)
    assert R.same_bits(got[:2], ref[:2]), f"{tag}: rows 0 / 1 / the counts differ"
    assert R.same_bits(got[2, :, -1], ref[2, :, -1]), f"{tag}: row 2's counts differ"
    fin = np.isfinite(ref[2, :, :-1])
    g2, r2 = got[2, :, :-1], ref[2, :, :-1]
    assert np.array_equal(np.isnan(g2), np.isnan(r2)) and np.array_equal(np.isposinf(g2), np.isposinf(r2)), \
        f"{tag}: a non-finite term left its own entry"
    w = R.worst(g2[fin], r2[fin], R.row2_bound(spectra, group, n_group)[fin])
    assert w <= 1, f"{tag}: row 2 err / bound {w}"
    return bool(R.same_bits(g2, r2))


@pytest.mark.parametrize("n_group,r", C.ACC_SHAPE)
@pytest.mark.parametrize("n", C.ACC_N)
def test_sigma_accumulate(n, n_group, r):
    a = C.acc_case(n, n_group, r)
    exact = []
    for tag, spectra, group in (("grouped", a.spectra, a.group), ("ungrouped", a.spectra, None),
                                ("nan", a.nan, a.group), ("nan ungrouped", a.nan, None)):
        got = noise.sigma_accumulate(T_(spectra), None if group is None else T_(group), n_group)
        again = noise.sigma_accumulate(T_(spectra), None if group is None else T_(group), n_group)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))
        exact.append(check_acc(got, spectra, group, n_group, f"n {n} ({n_group}, {r}) {tag}"))
    print(f"accumulate n {n} ({n_group}, {r}): row 2 bit-equal {exact}")


@pytest.mark.parametrize("n_group,r", C.ACC_SHAPE)
@pytest.mark.parametrize("a,b", C.ACC_SPLIT)
def test_sigma_accumulate_split(a, b, n_group, r):
    c = C.acc_case(a + b, n_group, r)
    s, g = T_(c.spectra), T_(c.group)
    one = noise.sigma_accumulate(s, g, n_group)
    acc = noise.sigma_accumulate(s[:a].contiguous(), g[:a].contiguous(), n_group)
    two = noise.sigma_accumulate(s[a:].contiguous(), g[a:].contiguous(), n_group, acc)
    assert two is acc and torch.equal(one, two)
    check_acc(two, c.spectra, c.group, n_group, f"split {a} + {b}")


def _stale(*shape):
    """leave a freed block of this size holding the sentinel, for the allocator to hand out next"""
    t = torch.full(shape, R.SENTINEL, dtype=torch.float32, device=DEV)
    del t


@pytest.mark.parametrize("n", C.ROWS_N)
def test_sig_rcp_rows(n):
    c = C.rows_case(n)
    nm = noise.NoiseModel(16, c.n_group, DEV, r=7, n_col=c.n_col)
    nm._set(np.zeros_like(c.rcp), c.rcp)
    _stale(5, n)
    got = nm.sig_rcp_rows(c.px, T_(c.group)).cpu().numpy()
    assert R.same_bits(got, R.rows_emu(c.rcp, c.group, c.iSig, 5))
    _stale(2, n)
    got = nm.sig_rcp_rows(c.px, None, n=2).cpu().numpy()
    assert R.same_bits(got, R.rows_emu(c.rcp, None, c.iSig, 2))


@pytest.mark.parametrize("with_ori", [True, False], ids=["ori", "no-ori"])
@pytest.mark.parametrize("N", C.SCALE_N)
def test_img_scale(N, with_ori):
    c = C.scale_case(N)
    for s in C.SCALE:
        img, ori = T_(c.img), T_(c.ori)
        noise.img_scale(img[1:4], ori[1:4] if with_ori else None, T_(s))
        img, ori = img.cpu().numpy(), ori.cpu().numpy()
        assert R.same_bits(img[[0, 4]], c.img[[0, 4]]) and R.same_bits(ori[[0, 4]], c.ori[[0, 4]])
        assert R.same_bits(img[1:4], R.scale_emu(c.img[1:4], s))
        assert R.same_bits(ori[1:4], R.scale_emu(c.ori[1:4], s) if with_ori else c.ori[1:4])


def test_zero_images_touch_nothing():
    """nImg = 0 on every entry point: status 0, every output as it was"""
    c, g = C.get("r3", False), up("r3", False)
    g2 = up("r3", True)
    p, st = ops._ptr, ops._stream(DEV)
    L = lib()
    n = len(c.img)
    outs = dict(ps=torch.full((n, c.r), R.SENTINEL, device=DEV),
                spectra=torch.full((n, 4, c.r), R.SENTINEL, device=DEV),
                norm=torch.full((n,), R.SENTINEL, dtype=torch.float64, device=DEV),
                acc=torch.full((3, 2, c.r + 1), R.SENTINEL, dtype=torch.float64, device=DEV),
                avg=torch.full((c.N, c.N // 2 + 1, 2), R.SENTINEL, dtype=torch.float64, device=DEV),
                pss=torch.full((c.r,), R.SENTINEL, dtype=torch.float64, device=DEV),
                rows=torch.full((n, c.px.n), R.SENTINEL, device=DEV),
                img=g.img.clone(), ori=g.ori.clone())
    before = {k: v.clone() for k, v in outs.items()}
    sp = g.sp
    tab = (p(sp.d_iCol), p(sp.d_iRow), p(sp.d_iPxl), p(sp.d_shellStart))
    rcp = torch.ones(2, c.r + 1, dtype=torch.float64, device=DEV)
    i_sig = T_(c.px.iSig)
    scale = torch.full((n,), 2.0, device=DEV)
    group = torch.zeros(n, dtype=torch.int32, device=DEV)
    calls = [
        L.thx_power_spectrum(p(g.img), 0, c.N, c.r, tab[2], tab[3], p(outs["ps"]), st),
        L.thx_residual_spectra(p(g.vols), c.vdim, c.pf, 2, p(g.img), p(g.ori), p(g.attr), p(g.rot), p(g.trans),
                               p(g.off), p(g.dF), p(g.cls), 0, c.N, c.r, *tab, p(outs["spectra"]),
                               p(outs["norm"]), 0.0, 2.5, st),
        L.thx_residual_spectra2d(p(g2.vols), c.vdim, c.pf, 2, p(g2.img), p(g2.ori), p(g2.attr), p(g2.rot),
                                 p(g2.trans), p(g2.off), p(g2.dF), p(g2.cls), 0, c.N, c.r, *tab,
                                 p(outs["spectra"]), p(outs["norm"]), 0.0, 2.5, st),
        L.thx_sigma_accumulate(p(outs["spectra"]), p(group), 0, c.r, 2, p(outs["acc"]), st),
        L.thx_sigma_init_accumulate(p(g.ori), 0, c.N, c.r, tab[2], tab[3], p(outs["avg"]), p(outs["pss"]), st),
        L.thx_sig_rcp_rows(p(rcp), 2, c.r + 1, p(group), p(i_sig), c.px.n, 0, p(outs["rows"]), st),
        L.thx_img_scale(p(outs["img"]), p(outs["ori"]), p(scale), 0, c.N, st),
    ]
    torch.cuda.synchronize()
    assert calls == [0] * len(calls), L.thx_last_error()
    for k, v in outs.items():
        assert R.same_bits(v.cpu().numpy(), before[k].cpu().numpy()), f"{k} was touched"
