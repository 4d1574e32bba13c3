"""The noise model on the GPU (csrc/noise.hip, thunder_amd/noise.py) against
the float64 restatement of tests/noise_ref.py: powerSpectrum, the four residual
spectra of Optimiser::allReduceSigma (src/Optimiser.cpp:6395-6709) in 3D and
2D, normCorrection's norm and rescale (:6201-6393), the per-group sums, the
finalised sig / sigRcp, initSigma (:5145-5243), allocPreCal's rows (:8060-8071)
and the rows' way into a local phase.

Images are written directly in Fourier space: CTF x phase x slice from the C
oracle on the disc plus independent complex noise on EVERY stored pixel --
column 0 below the axis included, so it is deliberately not Hermitian-
consistent with j > 0 -- and stronger garbage outside the disc, which has to be
ignored.

The bound on the spectra is relative, max(1e-5, 4 e32): 1e-5 is the project's
likelihood tolerance (the sigRcp-weighted sum of these shells is the dvp), e32
is the worst per-shell error of the same restatement evaluated in numpy
float32 against float64 on the same inputs, computed here and printed.
"""
import types

import numpy as np
import pytest
import torch

import noise_ref
from thunder_amd import noise, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PF = 2
N_IMG = 7
CLS = np.array([0, 1, 1, 0, 1, 0, 0], np.int32)
GROUP = np.array([0, 1, 0, 2, 1, 0, 1], np.int32)        # interleaved; group 2 has one image
N_GROUP = 3
DF = np.array([1.0, 1.02, 1.0, 0.97, 1.0, 1.0, 1.01])
NORM_RADII = (2.0, 9.5)          # a fractional bound: on the pixel radius, not on the shell
CASES = [(32, 10), (64, 31)]     # r below N/2 - 1; shells longer than one wave
SNRS = [0.5, 20.0]


def T_(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _classes2d(nK, N, seed):
    vdim = N * PF
    rng = np.random.default_rng(seed)
    out = np.empty((nK, vdim, vdim // 2 + 1), np.complex64)
    yy, xx = np.mgrid[:vdim, :vdim] - vdim // 2
    for k in range(nK):
        img = np.zeros((vdim, vdim))
        for _ in range(6):
            cx, cy = rng.uniform(-N / 4, N / 4, 2)
            img += rng.uniform(0.5, 1.5) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2)
                                                  / (2 * rng.uniform(1.0, 3.0) ** 2))
        out[k] = np.fft.rfft2(np.fft.ifftshift(img)) / vdim
    return out


_vols = {}


def volumes(N, two_d):
    key = (N, two_d)
    if key not in _vols:
        if two_d:
            _vols[key] = _classes2d(2, N, 40 + N)
        else:
            _vols[key] = np.stack([synth.projectee(synth.blob_volume(N, n_blobs=30, seed=s), PF)
                                   .numpy() for s in (1, 2)])
    return _vols[key]


def _noise(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


_cases = {}


def make_case(orc, N, r, snr, two_d, seed=3, noise_free=False, sigma2=None, zero_off=False):
    """One stack with its float64 reference and float32 error.  sigma2 [r]:
    the per-component noise variance per shell (the loop-closure case);
    otherwise the shell's signal power / snr."""
    key = (N, r, snr, two_d, seed, noise_free, sigma2 is not None, zero_off)
    if key in _cases:
        return _cases[key]
    vdim = N * PF
    vols = volumes(N, two_d)
    px = noise_ref.disc(orc, N, r, PF)
    rng = np.random.default_rng(seed + N + int(two_d))
    attr = synth.ctf_attrs(N_IMG, seed=seed + 5)
    rot = (np.stack([noise_ref.rot2(a) for a in rng.uniform(0, 2 * np.pi, N_IMG)]) if two_d
           else synth.uniform_quaternions(N_IMG, rng))
    trans = rng.standard_normal((N_IMG, 2)) * 2
    off = np.zeros((N_IMG, 2)) if zero_off else rng.standard_normal((N_IMG, 2)) * 1.5
    shape = (N_IMG, N, N // 2 + 1)
    img = np.zeros(shape, np.complex64)
    ori = np.zeros(shape, np.complex64)
    in_disc = np.zeros(N * (N // 2 + 1), bool)
    in_disc[px.iPxl] = True
    for l in range(N_IMG):
        P, ctf = noise_ref.slice_terms(orc, px, vols[CLS[l]], vdim, PF, rot[l], attr[l], DF[l], N)
        M = noise_ref.model(orc, px, P, ctf, trans[l], N, np.float32)
        Nn = noise_ref.model(orc, px, P, ctf, trans[l] - off[l], N, np.float32)
        if sigma2 is not None:
            amp = np.sqrt(sigma2)[px.iSig]
        else:
            pw = noise_ref.shell_means(M.real ** 2 + M.imag ** 2, px.iSig, r)
            amp = np.sqrt(pw / snr / 2)[px.iSig]
        for dst, sgn in ((img, M), (ori, Nn)):
            full = np.zeros(N * (N // 2 + 1), np.complex128)
            if not noise_free:
                full[~in_disc] = 3 * amp.max() * _noise(rng, np.count_nonzero(~in_disc))
                full[px.iPxl] = amp * _noise(rng, px.n)
            full[px.iPxl] += sgn
            dst[l] = full.reshape(N, N // 2 + 1).astype(np.complex64)
        if sigma2 is not None:
            ori[l] = img[l]
    c = types.SimpleNamespace(N=N, r=r, vdim=vdim, vols=vols, px=px, attr=attr, rot=rot,
                              trans=trans, off=off, img=img, ori=ori, two_d=two_d)
    args = (orc, px, r, vols, vdim, PF, img, ori, attr, rot, trans, off, DF, CLS, N, NORM_RADII)
    c.ref, c.ref_norm = noise_ref.residual_spectra(*args)
    r32, n32 = noise_ref.residual_spectra(*args, dtype=np.float32)
    if not noise_free:
        assert c.ref.min() > 0, "a zero-power shell: pick another seed"
        c.e32 = float(np.max(np.abs(r32 - c.ref) / c.ref))
        c.e32_norm = float(np.max(np.abs(n32 - c.ref_norm) / c.ref_norm))
    _cases[key] = c
    return c


def gpu_spectra(c, sp, norm=True):
    return noise.residual_spectra(T_(c.vols), T_(c.img), T_(c.ori), T_(c.attr), T_(c.rot),
                                  T_(c.trans), sp, PF, T_(c.off), T_(DF), T_(CLS),
                                  norm_radii=NORM_RADII if norm else None)


def stack_of(c):
    """what NoiseModel needs of an ingest.Stack"""
    return types.SimpleNamespace(N=c.N, imgFT=T_(c.img), oriFT=T_(c.ori), attr=T_(c.attr),
                                 r_mask=0.35 * c.N)


@pytest.mark.parametrize("N,r", CASES)
def test_power_spectrum(orc, N, r):
    c = make_case(orc, N, r, 0.5, False)
    sp = noise.SpectrumPixels(N, r, DEV)
    got = noise.power_spectrum(T_(c.ori), sp).cpu().numpy()
    ref = np.stack([noise_ref.power_spectrum(o, c.px, r) for o in c.ori])
    r32 = np.stack([noise_ref.power_spectrum(o, c.px, r, np.float32) for o in c.ori])
    e32 = np.max(np.abs(r32 - ref) / ref)
    err = np.max(np.abs(got - ref) / ref)
    print(f"power spectrum N={N} r={r}: gpu {err:.3e} e32 {e32:.3e}")
    assert err <= max(1e-5, 4 * e32)


@pytest.mark.parametrize("two_d", [False, True], ids=["3d", "2d"])
@pytest.mark.parametrize("snr", SNRS)
@pytest.mark.parametrize("N,r", CASES)
def test_residual_spectra_and_norm(orc, N, r, snr, two_d):
    c = make_case(orc, N, r, snr, two_d)
    sp = noise.SpectrumPixels(N, r, DEV)
    got, norm = gpu_spectra(c, sp)
    again, norm2 = gpu_spectra(c, sp)
    assert torch.equal(got, again) and torch.equal(norm, norm2)      # bit-identical runs
    got, norm = got.cpu().numpy(), norm.cpu().numpy()
    err = np.abs(got - c.ref) / c.ref
    rows = [float(err[:, q].max()) for q in range(4)]
    print(f"residual spectra N={N} r={r} snr={snr} {'2d' if two_d else '3d'}: gpu rows "
          + " ".join(f"{e:.3e}" for e in rows) + f" e32 {c.e32:.3e}")
    assert max(rows) <= max(1e-5, 4 * c.e32)
    en = float(np.max(np.abs(norm - c.ref_norm) / c.ref_norm))
    print(f"norm: gpu {en:.3e} e32 {c.e32_norm:.3e}")
    assert en <= max(1e-5, 4 * c.e32_norm)


def test_without_ori_and_defaults(orc):
    """oriFT NULL leaves row 1 alone; offS / dF / cls NULL mean 0 / 1 / class 0"""
    c = make_case(orc, 32, 10, 0.5, False)
    sp = noise.SpectrumPixels(32, 10, DEV)
    full, _ = gpu_spectra(c, sp, norm=False)
    s, n = noise.residual_spectra(T_(c.vols), T_(c.img), None, T_(c.attr), T_(c.rot), T_(c.trans),
                                  sp, PF, None, T_(DF), T_(CLS))
    assert n is None and torch.equal(s[:, 1], torch.zeros_like(s[:, 1]))
    assert torch.equal(s[:, [0, 2, 3]], full[:, [0, 2, 3]])
    d, _ = noise.residual_spectra(T_(c.vols[0]), T_(c.img), T_(c.ori), T_(c.attr), T_(c.rot),
                                  T_(c.trans), sp, PF)
    e, _ = noise.residual_spectra(T_(c.vols), T_(c.img), T_(c.ori), T_(c.attr), T_(c.rot),
                                  T_(c.trans), sp, PF, T_(np.zeros((N_IMG, 2))), T_(np.ones(N_IMG)),
                                  T_(np.zeros(N_IMG, np.int32)))
    assert torch.equal(d, e)
    bad = CLS.copy()
    bad[2] = 2                       # outside the two projectees: NaN, no gather
    b, _ = noise.residual_spectra(T_(c.vols), T_(c.img), T_(c.ori), T_(c.attr), T_(c.rot),
                                  T_(c.trans), sp, PF, T_(c.off), T_(DF), T_(bad))
    assert torch.isnan(b[2]).all() and torch.equal(b[[0, 1, 3, 4, 5, 6]], full[[0, 1, 3, 4, 5, 6]])


def test_noise_free_residual_vanishes(orc):
    """imgFT = the float32 signal itself: every shell of |img - M|^2 is below
    1e-9 of |img|^2 ((32 * 2^-24)^2 rounded up: 32 FP32 roundings of amplitude)"""
    for two_d in (False, True):
        c = make_case(orc, 32, 15, 20.0, two_d, noise_free=True)
        sp = noise.SpectrumPixels(32, 15, DEV)
        got, _ = gpu_spectra(c, sp, norm=False)
        got = got.cpu().numpy()
        print("noise-free: max row0/row3", float((got[:, 0] / got[:, 3]).max()),
              "row1/row3", float((got[:, 1] / got[:, 3]).max()))
        assert np.all(got[:, 0] < 1e-9 * got[:, 3])
        assert np.all(got[:, 1] < 1e-9 * got[:, 3])


@pytest.mark.parametrize("N,r", CASES)
def test_sigma_accumulate(orc, N, r):
    c = make_case(orc, N, r, 0.5, False)
    sp = noise.SpectrumPixels(N, r, DEV)
    spectra, _ = gpu_spectra(c, sp, norm=False)
    g = T_(GROUP)
    one = noise.sigma_accumulate(spectra, g, N_GROUP)
    ref = noise_ref.sigma_sums(spectra.cpu().numpy(), GROUP, N_GROUP)
    assert np.allclose(one.cpu().numpy(), ref, rtol=1e-12, atol=0)

    def split():
        acc = noise.sigma_accumulate(spectra[:4].contiguous(), g[:4].contiguous(), N_GROUP)
        return noise.sigma_accumulate(spectra[4:].contiguous(), g[4:].contiguous(), N_GROUP, acc)
    a, b = split(), split()
    assert torch.equal(a, b)                                   # bit-identical
    assert np.allclose(a.cpu().numpy(), one.cpu().numpy(), rtol=1e-12, atol=0)
    # ungrouped: everything in row 0
    u = noise.sigma_accumulate(spectra, None, N_GROUP).cpu().numpy()
    assert np.allclose(u, noise_ref.sigma_sums(spectra.cpu().numpy(), None, N_GROUP), rtol=1e-12,
                       atol=0)
    assert np.all(u[:, 1:] == 0) and np.all(u[:, 0, r] == N_IMG)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("two_d", [False, True], ids=["3d", "2d"])
@pytest.mark.parametrize("N,r", CASES)
def test_update_end_to_end(orc, N, r, two_d, grouped):
    c = make_case(orc, N, r, 20.0, two_d)
    n_col = N // 2                      # maxR + 1: for r = 10 the column extension runs
    nm = noise.NoiseModel(N, N_GROUP, DEV, r=r, n_col=n_col)
    st = stack_of(c)
    alpha = nm.alpha_of(st)
    assert alpha == pytest.approx(np.sqrt(np.pi) * 0.35)
    group = T_(GROUP) if grouped else None
    sig, rcp = nm.update(st, T_(c.vols), T_(c.rot), T_(c.trans), PF, T_(c.off), T_(DF), T_(CLS),
                         group)
    rsig, rrcp = noise_ref.sigma_finalise(
        noise_ref.sigma_sums(c.ref, GROUP if grouped else None, N_GROUP), n_col, alpha, grouped)
    bound = max(1e-5, 4 * c.e32)
    es = float(np.max(np.abs(sig[:, :-1] - rsig[:, :-1]) / np.abs(rsig[:, :-1])))
    er = float(np.max(np.abs(rcp[:, :-1] - rrcp[:, :-1]) / np.abs(rrcp[:, :-1])))
    print(f"update N={N} r={r} grouped={grouped}: sig {es:.3e} sigRcp {er:.3e} bound {bound:.3e}")
    assert es <= bound and er <= bound
    assert np.all(sig[:, -1] == 0) and np.all(rcp[:, -1] == 0)
    # allocPreCal's rows, exactly
    px = ops.PixelSet(N, PF, min(r, 12), 1, device=DEV)
    rows = nm.sig_rcp_rows(px, group, n=N_IMG).cpu().numpy()
    g = GROUP if grouped else np.zeros(N_IMG, np.int32)
    assert np.array_equal(rows, rcp[g][:, px.iSig].astype(np.float32))


def test_loop_closure(orc):
    """Noise of known per-shell variance around the model at the true poses,
    imgFT = oriFT, alpha = 1, one group: sig[u] estimates sigma^2[u] as a
    chi-square mean over 7 count[u] complex pixels, relative deviation
    1 / sqrt(7 count[u]); 5 deviations for the shells with count >= 20."""
    N, r = 32, 15
    sigma2 = 0.5 + 0.1 * np.arange(r)
    c = make_case(orc, N, r, 0.0, False, seed=4, sigma2=sigma2, zero_off=True)
    count = np.bincount(c.px.iSig, minlength=r)
    big = count >= 20
    assert big.sum() >= 5
    tol = 5 / np.sqrt(N_IMG * count)
    rsig, _ = noise_ref.sigma_finalise(noise_ref.sigma_sums(c.ref, None, 1), r + 1, 1.0, False)
    assert np.all(np.abs(rsig[0, :r] - sigma2)[big] <= (tol * sigma2)[big])   # the seed is sound
    nm = noise.NoiseModel(N, 1, DEV)
    sig, _ = nm.update(stack_of(c), T_(c.vols), T_(c.rot), T_(c.trans), PF, None, T_(DF), T_(CLS),
                       None, alpha=1.0)
    dev = np.abs(sig[0, :r] - sigma2) / sigma2
    print("loop closure: worst deviation / allowance", float((dev / tol)[big].max()))
    assert np.all(dev[big] <= tol[big])


@pytest.mark.parametrize("N,r", [(32, 15), (64, 31)])
def test_init_from(orc, N, r):
    c = make_case(orc, N, r, 0.5, False)
    nm = noise.NoiseModel(N, N_GROUP, DEV)
    assert nm.r == r and nm.n_col == r + 1
    st = stack_of(c)
    sig, rcp = nm.init_from(st)
    # the accumulators against FP64 sums of the device's own terms
    ps = noise.power_spectrum(st.oriFT, nm.sp).double().sum(0).cpu().numpy()
    assert np.allclose(nm.ps_sum.cpu().numpy(), ps, rtol=1e-12, atol=0)
    avg = torch.view_as_real(st.oriFT).double().sum(0).cpu().numpy()
    assert np.allclose(nm.avg_sum.cpu().numpy(), avg, rtol=0, atol=1e-12 * np.abs(avg).max())
    # accumulating in two calls continues the sums
    a, p = noise.sigma_init_accumulate(st.oriFT[:3].contiguous(), nm.sp)
    a, p = noise.sigma_init_accumulate(st.oriFT[3:].contiguous(), nm.sp, a, p)
    assert np.allclose(a.cpu().numpy(), avg, rtol=0, atol=1e-12 * np.abs(avg).max())
    assert np.allclose(p.cpu().numpy(), ps, rtol=1e-12, atol=0)
    rs, rr = noise_ref.init_finalise(*noise_ref.init_sums(c.ori, c.px, r), N_IMG, c.px, r, N_GROUP,
                                     r + 1)
    es = float(np.max(np.abs(sig[:, :-1] - rs[:, :-1]) / np.abs(rs[:, :-1])))
    print(f"init sigma N={N}: {es:.3e}")
    assert es <= 1e-5
    assert np.max(np.abs(rcp[:, :-1] - rr[:, :-1]) / np.abs(rr[:, :-1])) <= 1e-5


@pytest.mark.parametrize("n", [7, 6])
def test_norm_correction(orc, n):
    """after the rescale every recomputed norm equals the median; an even count
    takes the mean of the two middle values"""
    c = make_case(orc, 32, 10, 0.5, False)
    nm = noise.NoiseModel(32, 1, DEV, r=10)
    st = types.SimpleNamespace(N=32, imgFT=T_(c.img[:n]), oriFT=T_(c.ori[:n]),
                               attr=T_(c.attr[:n]), r_mask=11.0)
    pose = dict(pf=PF, dF=T_(DF[:n]), cls=T_(CLS[:n]))
    args = (st, T_(c.vols), T_(c.rot[:n]), T_(c.trans[:n]), *NORM_RADII)
    before_ori = st.oriFT.clone()
    norm, m = nm.norm_correction(*args, **pose)
    norm = norm.cpu().numpy()
    s = np.sort(norm)
    assert m == (s[3] if n == 7 else (s[2] + s[3]) / 2)
    # the model is not rescaled, so the residual's norm moves only where the
    # image dominates it: check the rescale itself, then the norms of the
    # scaled images against the restatement on the scaled images
    scale = np.sqrt(m / norm).astype(np.float32)
    assert torch.equal(st.oriFT, before_ori * T_(scale)[:, None, None])
    assert torch.equal(st.imgFT, T_(c.img[:n]) * T_(scale)[:, None, None])
    after = nm.norms(*args, **pose).cpu().numpy()
    ref, ref_n = noise_ref.residual_spectra(orc, c.px, 10, c.vols, c.vdim, PF,
                                            st.imgFT.cpu().numpy(), st.oriFT.cpu().numpy(),
                                            c.attr[:n], c.rot[:n], c.trans[:n], c.off[:n], DF[:n],
                                            CLS[:n], 32, NORM_RADII)
    assert np.max(np.abs(after - ref_n) / ref_n) <= 1e-5


def test_norm_correction_equalises_pure_noise(orc):
    """with no model (a zero projectee) the norm is the image's own power in
    the annulus, so after the rescale every norm equals the median at 1e-5"""
    c = make_case(orc, 32, 10, 0.5, False)
    nm = noise.NoiseModel(32, 1, DEV, r=10)
    st = stack_of(c)
    zero = torch.zeros_like(T_(c.vols))
    args = (st, zero, T_(c.rot), T_(c.trans), *NORM_RADII)
    _, m = nm.norm_correction(*args, pf=PF, cls=T_(CLS))
    after = nm.norms(*args, pf=PF, cls=T_(CLS)).cpu().numpy()
    print("norm correction: worst |norm/median - 1|", float(np.max(np.abs(after / m - 1))))
    assert np.max(np.abs(after / m - 1)) <= 1e-5


def test_rows_feed_local_phase(orc):
    """the updated sigRcp rows through one local phase (box 32): its dvp matches
    the oracle's given the same rows at the likelihood tolerance"""
    N, r = 32, 15
    c = make_case(orc, N, r, 0.5, False)
    nm = noise.NoiseModel(N, N_GROUP, DEV)
    st = stack_of(c)
    nm.update(st, T_(c.vols), T_(c.rot), T_(c.trans), PF, T_(c.off), T_(DF), T_(CLS), T_(GROUP))
    px = ops.PixelSet(N, PF, 12, 1, device=DEV)
    opx = orc.pixel_set(N, PF, 12, 1)
    assert np.array_equal(px.iPxl, opx.iPxl)
    rows = nm.sig_rcp_rows(px, T_(GROUP))
    from thunder_amd import ingest
    dat = ingest.gather(st.imgFT, px.iPxl)
    ctf = ops.ctf(st.attr, px)
    nR, nT = 6, 5
    rng = np.random.default_rng(21)
    quat = synth.uniform_quaternions(N_IMG * nR, rng).reshape(N_IMG, nR, 4)
    trans = rng.standard_normal((N_IMG, nT, 2)) * 2
    pC, pR, pT = np.ones(N_IMG), np.full((N_IMG, nR), 1 / nR), np.full((N_IMG, nT), 1 / nT)
    vol = T_(c.vols[0])
    *_, d = ops.local_phase(vol, T_(quat), T_(trans), T_(pC), T_(pR), T_(pT), dat, ctf, rows, px,
                            want_dvp=True)
    d, dat, ctf, rows = (x.cpu().numpy() for x in (d, dat, ctf, rows))
    assert np.all(rows < 0) and np.all(np.isfinite(rows))
    for l in range(N_IMG):
        *_, rd = orc.local_phase(c.vols[0], c.vdim, PF, quat[l], trans[l], 1.0, pR[l], pT[l],
                                 dat[l], ctf[l], rows[l], opx, N)
        assert np.max(np.abs(d[l] - rd) / np.abs(rd)) < 1e-5
