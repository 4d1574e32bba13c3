"""The box-less local-phase kernels visit the step-compacted order
(thx_step_compact_order) instead of the tile order.  A removed step adds
exactly zero and A_l keeps the tile order's summation (k_image_const), so with
the compaction (default) and without (THX_STEP_COMPACTION=0) a phase and the
whole driver return the same bits."""
import numpy as np
import pytest
import torch

from thunder_amd import expectation as ex
from thunder_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N_IMG, N_T = 3, 9
# all-padding steps mid-order in both; (64, 20) has an odd group count (41),
# (32, 6) four mostly partial groups (tests/test_step_compaction.py)
SHAPES = [(64, 20), (32, 6)]


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"box{s[0]}_rU{s[1]}")
def stack(request):
    N, rU = request.param
    px = ops.PixelSet(N, 2, rU, 1, device=DEV)
    vol = synth.projectee(synth.blob_volume(N, seed=90 + N, device=DEV), 2)
    rng = np.random.default_rng(91 + N)
    dat = (rng.standard_normal((N_IMG, px.n)) + 1j * rng.standard_normal((N_IMG, px.n))).astype(np.complex64)
    ctf = rng.uniform(-1, 1, (N_IMG, px.n)).astype(np.float32)
    sig = rng.uniform(0.5, 2.0, (N_IMG, px.n)).astype(np.float32)
    R = ops.ypair_ball_radius(px)
    return dict(px=px, vol=vol, dat=T(dat), ctf=T(ctf), sig=T(sig), rng_seed=92 + N,
                ypair=ops.volume_ypair(vol), cells=ops.volume_cells(vol),
                ball=ops.volume_ypair_ball(vol, R), R=R)


def test_device_compaction_is_the_host_compaction(stack):
    px = stack["px"]
    got = ops.step_compact_order_device(px.d_order).cpu().numpy()
    assert np.array_equal(got, ops.step_compact_order(px.order))
    assert len(got) < len(px.order) or len(px.order) % 32 == 0


# kernel: how the phase is called -> the route a routed call must report
KERNELS = {
    "ypair": (lambda s: dict(ypair=s["ypair"]), None),                      # whole y-pair copy
    "ball": (lambda s: dict(routed=True, ball=s["ball"], ball_r=s["R"]), 2),  # compact ball
    "ypair_routed": (lambda s: dict(routed=True, ypair=s["ypair"]), 2),
    "nobox": (lambda s: dict(routed=True), 1),                              # STAGE = false
    "cells": (lambda s: dict(cells=s["cells"]), None),
}


@pytest.mark.parametrize("mLR", [125, 37])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_phase_is_bit_identical(stack, monkeypatch, kernel, mLR):
    s = stack
    rng = np.random.default_rng(s["rng_seed"] + mLR)
    # rotations all over the sphere: no patch neighbourhood fits an LDS box, so
    # the route takes a box-less kernel at either size
    quat = synth.uniform_quaternions(N_IMG * mLR, rng).reshape(N_IMG, mLR, 4)
    trans = rng.standard_normal((N_IMG, N_T, 2)) * 2
    args = (T(quat), T(trans), T(np.ones(N_IMG)), T(np.full((N_IMG, mLR), 1.0 / mLR)),
            T(np.full((N_IMG, N_T), 1.0 / N_T)), s["dat"], s["ctf"], s["sig"], s["px"])
    kw, route = KERNELS[kernel]
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("THX_STEP_COMPACTION", flag)
        r = ops.local_phase(s["vol"], *args, want_dvp=True, **kw(s))
        if route is not None:
            assert r[5] == route, (flag, r[5])
        outs.append([x.clone() for x in r[:5]])
    for name, a, b in zip(("wC", "wR", "wT", "baseline", "dvp"), *outs):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_driver_is_bit_identical(monkeypatch):
    """Box 64, 16 images, 2 phases of a global search at the bench's SNR (wide
    clouds: the route takes the y-pair kernel, asserted): the same clouds,
    priors, scores, classes and phase counts with the compaction on and off."""
    from bench import make_stack
    N, rU, n = 64, 20, 16
    vol = synth.projectee(synth.blob_volume(N, seed=95, device=DEV), 2)
    px, dat, ctf, sig, *_ = make_stack(N, 2, rU, 1, n, DEV, seed=96, vol=vol)
    gset = synth.global_sample_set(1500, seed=97)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("THX_STEP_COMPACTION", flag)
        e = ex.Expectation(vol, px, gset, n_phase=2, seed=14)
        routes = e.track_routes(2)
        outs.append([x.clone() for x in e.run(dat, ctf, sig)])
        assert routes.cpu().tolist() == [2, 2], (flag, routes.cpu().tolist())
    for a, b in zip(*outs):
        assert torch.equal(a, b)
