"""The oracle's own error budget at the metric configuration C3 (CPU).

SURVEY §7's parity definition compares the GPU with the restatement, which
evaluates the reference's direct form sum_i s |d - c T P|^2 in FP32
(src/Optimiser.cpp:9187-9213, orc_logdatavs).  How far that FP32 evaluation
itself sits from the exact sum bounds what any GPU-vs-oracle tolerance can
claim.  Here the oracle's dvp (orc.dvp_global) is compared with a float64
evaluation of the same sum from the same FP32 operands (the oracle's FP32
projections P and phase table T, the FP32 images, CTF and sigRcp), at C3's
shape (box 256, pf 2, rU 24 -> nPxl 870, all 151 translations, a subset of
the 2000 rotations that holds the SNR-20 images' true poses), at the bench's
SNR 0.05 and at SNR 20.

Measured (recorded in DESIGN.md §2): the oracle's dvp are within ~2e-6
relative of the float64 sum (|dvp| ~ 400-30 000), and that moves the
normalised marginals exp(dvp - max) by up to ~9e-4 relative at SNR 0.05 --
so the GPU-vs-oracle marginal tolerance of 1e-3 (test_gpu_configs.py) is the
oracle's own budget, and 1e-4 against the oracle is not supportable.  The
GPU side of the same budget (GPU dvp and marginals against float64) is
test_gpu_configs.py::test_c3_scan_error_budget_against_float64.
"""
import numpy as np
import pytest
import torch

from scan_ref import dvp64
from thunder_amd import synth

N, PF, RU, RL = 256, 2, 24, 1


def c3_budget_stack(orc, vol, px, gset, rsel, snr, nImg, seed):
    """nImg CTF-modulated images: at SNR > 1 at grid poses (a rotation of
    rsel, a translation of the set), else at random poses; built with the
    oracle's projection, phase shift and CTF."""
    q, t = gset[0], gset[1]
    rng = np.random.default_rng(seed)
    ir = rsel[rng.integers(0, len(rsel), nImg)]
    it = rng.integers(0, len(t), nImg)
    attrs = synth.ctf_attrs(nImg, seed=seed + 1)
    ctf = np.stack([orc.ctf(px, a, N) for a in attrs]).astype(np.float32)
    sig = []
    for l in range(nImg):
        qt = q[ir[l]] if snr > 1 else synth.uniform_quaternions(1, rng)[0]
        tt = t[it[l]] if snr > 1 else rng.standard_normal(2) * 3
        p = orc.project3d(vol, N * PF, PF, orc.rotate3d(qt), px)
        sig.append(ctf[l] * p * orc.translate(px, *tt, N))
    dat, sg = synth.noisy_images(torch.from_numpy(np.stack(sig)), px.iSig, N // 2 + 1, snr=snr,
                                 seed=seed + 3)
    return dat.numpy(), ctf, sg.numpy().astype(np.float32)


def dvp_float64(P, Tt, dat, ctf, sig):
    """sum_i s |d - c (T P)|^2 in float64 from FP32 operands: P [nR, nPxl],
    Tt [nT, nPxl] complex, images [nImg, nPxl]; -> [nImg, nR, nT]
    (scan_ref.dvp64, the reference of the scan's edge tests too)."""
    return dvp64(P, Tt, dat, ctf, sig)


def marginals(d, pR, pT):
    """(wR [nImg, nR], wT [nImg, nT]) of exp(dvp - max) in float64."""
    e = np.exp(d - d.max(axis=(1, 2), keepdims=True))
    return e @ pT, np.einsum("lrt,r->lt", e, pR)


def max_marginal_rel(got, ref):
    m = ref >= 1e-4 * ref.max(axis=-1, keepdims=True)
    return float((np.abs(got - ref)[m] / ref[m]).max())


@pytest.fixture(scope="module")
def c3cpu(orc):
    vol = synth.projectee(synth.blob_volume(N, seed=1), PF).numpy()
    px = orc.pixel_set(N, PF, RU, RL)
    gset = synth.global_sample_set(2000, seed=2)
    rsel = np.sort(np.random.default_rng(5).choice(2000, 120, replace=False))
    P = np.stack([orc.project3d(vol, N * PF, PF, orc.rotate3d(gset[0][r]), px) for r in rsel])
    Tt = np.stack([orc.translate(px, *tr, N) for tr in gset[1]])
    return dict(vol=vol, px=px, gset=gset, rsel=rsel, P=P, Tt=Tt)


@pytest.mark.parametrize("snr", [0.05, 20.0])
def test_oracle_dvp_budget_at_c3(orc, c3cpu, snr):
    s = c3cpu
    px, (q, t, pR, pT), rsel = s["px"], s["gset"], s["rsel"]
    assert px.n == 870 and len(t) == 151
    dat, ctf, sig = c3_budget_stack(orc, s["vol"], px, s["gset"], rsel, snr, 3, 70)
    d = orc.dvp_global(s["vol"], N * PF, PF, q[rsel], t, dat, ctf, sig, px, N).astype(np.float64)
    ref = dvp_float64(s["P"], s["Tt"], dat, ctf, sig)
    rel = np.abs(d - ref) / np.abs(ref)
    # the FP32 direct form: ~1e-6 relative (870 terms of magnitude ~|dvp| /
    # 870 summed in order, each with a few FP32 roundings)
    assert rel.max() < 5e-6, rel.max()
    pRs = np.full(len(rsel), 1.0 / len(rsel))
    wR, wT = marginals(d, pRs, pT)
    rR, rT = marginals(ref, pRs, pT)
    mr = max(max_marginal_rel(wR, rR), max_marginal_rel(wT, rT))
    # the oracle's marginals sit within 1e-3 of the exact ones -- the bound
    # the GPU-vs-oracle marginal tests use; at SNR 0.05 they use most of it
    # (|dvp| ~ 500: 2e-6 relative is 1e-3 in log-weight)
    assert mr < 1e-3, mr
    if snr < 1:
        assert mr > 1e-4, mr   # 1e-4 against the oracle would be below its own error
