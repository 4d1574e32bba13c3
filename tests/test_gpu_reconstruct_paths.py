"""The reconstruction solve on both balancing loops, at every stopping rule and
option, against the float64 restatement (tests/recon_ref.py).

thx_reconstruct_weights returns the balanced W and runs either loop on
request; thx_reconstruct gives the map and its transform.  Each case builds
T from one of recon_ref.sampling_density's families (left non-symmetric on the
kx = 0 and kx = vdim/2 planes) and F = T x white noise, runs the restatement in
float64 and in float32, and holds the device to 8 x the float32 restatement's
own error e32 in each metric: two correct float32 solves with different FFT
factorisations and summation orders differ by small constant factors, a
1e-5-class defect by far more.

Admissibility is asserted first, so an input that could stop elsewhere or
amplify rounding fails instead of passing vacuously: every ratio
diff[m] / diff[m-1] of the float64 run at least 0.01 from 0.95, every diff at
least 1 % from 1e-2, float32 and float64 stop at the same iteration, and
e32 <= 1e-5 in every metric.

Inputs were searched on the CPU with the two restatements.  What the search
found, and what therefore is not here:
  * holes is not robustly admissible anywhere: its float32 W differs from
    float64 by 1.0e-5 ... 3.6e-5 (max relative, 20 seeds at (16, 2); 2.6e-5
    ... 5.4e-5 at (16, 3) and (32, 1); 0.9e-5 ... 1.2e-5 at (32, 2), on one
    side of the cap or the other with the CPU's FFT library).  The cap of 30
    is reached by decades inputs instead: under method 0 on each loop, and on
    both loops at once in the cross-check.
  * box (20, 2), vdim 40: the real-space kernel table is looked up at
    round(|r|^2 / vdim^2 / 1e-5) = round(62.5 |r|^2), an exact tie at every
    odd |r|^2, resolved by the rounding of two divisions.  Float32 and float64
    pick different entries at half of the voxels, e32 of W is 1.7e-5 for
    every seed and T, and no input is admissible.  (22, 2) -- vdim 44, nc 23,
    no ties -- takes its place under the bar, and (20, 2) is held to
    8 x e32 without the cap in a test of its own.  At vdim 400 an eighth of
    the voxels tie and e32 of W is 8e-6.
"""
import json

import numpy as np
import pytest
import torch

import recon_ref
from thunder_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E32_CAP = 1e-5
BAR = 8.0

# shells 5 .. 8 hold values past both clamps; long enough for box 32
FSC_EDGES = np.array([0.95, 0.9, 0.85, 0.8, 0.75, 1.5, -0.2, 1.0, 0.0, 0.5, 0.45, 0.4, 0.35, 0.3,
                      0.25, 0.2, 0.15])
FSC = np.linspace(0.95, 0.2, 17)


def _stop_kind(it, diffs):
    if diffs[-1] < 1e-2:
        return "threshold"
    return "cap" if it == 30 else "no-decrease"


def reference(N, pf, T, seed, kw, smooth, cap=True):
    """The float64 and float32 restatements of one case (on the device from
    vdim 128), admissibility asserted.  T: float64 numpy, rounded to float32
    here as the device receives it."""
    vdim = N * pf
    dev = DEV if vdim >= 128 else torch.device("cpu")
    T = torch.as_tensor(T.astype(np.float32), device=dev)
    F = recon_ref.white_data(T.double(), seed, dev).to(torch.complex64)
    r64 = recon_ref.reconstruct(F, T, N, pf, dtype=torch.float64, **kw)
    r32 = recon_ref.reconstruct(F, T, N, pf, dtype=torch.float32, **kw)
    maxR = recon_ref.max_r(N, 1.9, kw.get("max_radius", 0))
    inside = recon_ref.ft_quad(vdim, dev) < (maxR * pf) ** 2
    e32 = recon_ref.solve_errors((r32[0], r32[1], r32[4]), (r64[0], r64[1], r64[4]), inside)
    ft64 = torch.fft.rfftn(r64[0])
    if smooth:
        e32["shells"] = float(recon_ref.shell_errors(torch.fft.rfftn(r32[0]), ft64, N, maxR).max())
    ratio, thres = recon_ref.stop_margins(r64[4])
    fig = dict(N=N, pf=pf, it=r64[3], it32=r32[3], ratio_margin=ratio, thres_margin=thres, e32=e32)
    print("RECON_REF", json.dumps(fig))      # the figures of DESIGN.md section 2
    assert r32[3] == r64[3], fig
    assert ratio >= 0.01 and thres >= 0.01, fig
    if cap:
        assert all(v <= E32_CAP for v in e32.values()), fig
    assert all(v > 0 for v in e32.values()), fig
    return dict(F=F, T=T, map=r64[0], W=r64[1], T_after=r64[2], it=r64[3], diffs=r64[4], ft=ft64,
                inside=inside, maxR=maxR, e32=e32, dev=dev)


def check_weights(ref, N, pf, kw, method, even, label, exact_T=False):
    """thx_reconstruct_weights against the float64 W, diffs, iteration count
    and T as the solve leaves it; twice, for bit-identical results."""
    T_in = ref["T"].to(DEV)
    runs = []
    for _ in range(2):
        T = T_in.clone()
        W, it, diffs = ops.reconstruct_weights(T, N, pf, method=method, **kw)
        runs.append((W, it, diffs, T))
    W, it, diffs, T_after = runs[0]
    assert runs[1][1] == it and runs[1][2] == diffs and torch.equal(runs[1][0], W)
    assert torch.equal(runs[1][3], T_after)
    W = W.to(ref["dev"])
    inside = ref["inside"]
    err = recon_ref.solve_errors((ref["map"], W, diffs), (ref["map"], ref["W"], ref["diffs"]), inside)
    del err["map"]
    want_T = ref["T_after"]
    if even:
        want_T = recon_ref.hermitian_plane_average(want_T)
    err_T = float(((T_after.to(ref["dev"]).double() - want_T).abs() / want_T).max())
    print("RECON_DEV", json.dumps(dict(case=label, method=method, it=it, err=err, T_after=err_T,
                                       ratio={k: err[k] / ref["e32"][k] for k in err})))
    assert it == ref["it"]
    assert torch.all(W[~inside] == 0)
    for k, v in err.items():
        assert v <= BAR * ref["e32"][k], (k, v, ref["e32"][k])
    assert err_T <= 1e-6
    if exact_T:      # nothing to divide: the inner columns are the input's, floored
        assert torch.equal(T_after[:, :, 1:-1], torch.clamp(T_in, min=1e-25)[:, :, 1:-1])
    return W, it, diffs


def check_map(ref, N, pf, kw, smooth, label):
    """thx_reconstruct (the solve's own choice of loop) against the float64
    map, its transform per shell, diffs and iteration count; twice."""
    vdim = N * pf
    runs = []
    for _ in range(2):
        hm = ops.HalfMap(vdim, DEV)
        hm.F.copy_(ref["F"])
        hm.T.copy_(ref["T"])
        runs.append(ops.reconstruct(hm, N, pf, **kw))
    dst, ft, it, diffs = runs[0]
    assert torch.equal(runs[1][0], dst) and runs[1][2] == it and runs[1][3] == diffs
    err = recon_ref.solve_errors((dst.to(ref["dev"]), ref["W"], diffs),
                                 (ref["map"], ref["W"], ref["diffs"]), ref["inside"])
    del err["W"]
    if smooth:
        err["shells"] = float(recon_ref.shell_errors(ft.to(ref["dev"]), ref["ft"], N, ref["maxR"]).max())
    print("RECON_DEV", json.dumps(dict(case=label, method="map", it=it, err=err,
                                       ratio={k: err[k] / ref["e32"][k] for k in err})))
    assert it == ref["it"]
    for k, v in err.items():
        assert v <= BAR * ref["e32"][k], (k, v, ref["e32"][k])
    return diffs


def run_case(N, pf, family, seed, p=0.0, kw=None, stop=None, cap=True, exact_T=False, tag=""):
    kw = kw or {}
    vdim = N * pf
    smooth = family == "smooth"
    even = vdim in (64, 128, 256, 512) and kw.get("grid_corr", True)
    T = recon_ref.sampling_density(family, vdim, seed, p)
    if "fsc" in kw:
        # pre-multiplied by the MAP factor: the balancing sees the smooth T
        # whatever the FSC (a 1000-fold step of T between shells, as a clamped
        # FSC makes, amplifies rounding past any float32 bar)
        maxR = recon_ref.max_r(N, 1.9, kw.get("max_radius", 0))
        T = T * recon_ref.map_factor(vdim, pf, maxR, kw["fsc"], kw.get("join_half", False)).numpy()
    ref = reference(N, pf, T, seed + 1000, kw, smooth, cap)
    if stop is not None:
        assert _stop_kind(ref["it"], ref["diffs"]) == stop, (ref["it"], ref["diffs"][-3:])
    label = f"{N}x{pf} {family} {seed} {tag}".strip()
    _, it, diffs = check_weights(ref, N, pf, kw, 0, even, label, exact_T)
    diffs_map = check_map(ref, N, pf, kw, smooth, label)
    assert diffs_map == diffs        # the two entry points run the same solve
    return ref


# ------------------------------------------------------- the 3D-transform loop
@pytest.mark.parametrize("N,pf", [(16, 2), (22, 2), (16, 3), (32, 1), (200, 2)])
def test_transform_loop_smooth(N, pf):
    """vdim 32 (a power of two below the even range), 44 (nc 23), 48 (u / pf
    at pf 3), 32 at pf 1, 400 (configuration C4): stops below 1e-2."""
    run_case(N, pf, "smooth", 0, stop="threshold")


def test_transform_loop_tie_box():
    """(20, 2), vdim 40, nc 21: the kernel-table lookup ties at every odd
    |r|^2 (module docstring), so e32 of W is 1.7e-5 whatever the input and the
    cap cannot hold; everything else is asserted, against 8 x e32."""
    ref = run_case(20, 2, "smooth", 0, stop="threshold", cap=False)
    assert ref["e32"]["W"] > E32_CAP     # else this case belongs under the cap


def test_transform_loop_no_decrease():
    """decades p = 1 at (16, 3): ends at iteration 11 by two diffs in a row
    not below 0.95 x the previous (ratio margin 0.016)."""
    ref = run_case(16, 3, "decades", 2, p=1.0, stop="no-decrease")
    assert 10 < ref["it"] < 30


def test_transform_loop_cap():
    """decades p = 0.9 at (32, 1): still at 1.7e-2 after 30 iterations."""
    run_case(32, 1, "decades", 0, p=0.9, stop="cap")


# ------------------------------------------------------ the even half-grid loop
@pytest.mark.parametrize("N,pf,seed", [(64, 2, 0), (32, 4, 0), (128, 2, 1), (64, 1, 0)])
def test_even_loop_smooth(N, pf, seed):
    """even_iteration_n<128> (at pf 2 and 4), <256>, and <64> at pf 1.  (Seed
    0 at (128, 2) comes within 0.7 % of 1e-2 at its last iteration.)"""
    run_case(N, pf, "smooth", seed, stop="threshold")


def test_even_loop_no_decrease():
    """decades p = 1 at (16, 4), vdim 64: ends at iteration 11 (ratio margin
    0.037).  None of 96 decades inputs at (32, 2) and (64, 1) was admissible
    with this ending."""
    ref = run_case(16, 4, "decades", 57, p=1.0, stop="no-decrease")
    assert 10 < ref["it"] < 30


def test_even_loop_cap():
    """decades p = 1 at (64, 1), vdim 64: 1.7e-2 after 30 iterations."""
    run_case(64, 1, "decades", 4, p=1.0, stop="cap")


# ------------------------------------------------------------- the two loops
@pytest.mark.parametrize("N,pf,family,seed,p,stop", [(32, 2, "smooth", 0, 0.0, "threshold"),
                                                     (32, 2, "decades", 4, 1.0, "cap"),
                                                     (64, 2, "smooth", 0, 0.0, "threshold")])
def test_both_loops_on_the_same_input(N, pf, family, seed, p, stop):
    """Method 1 (3D transforms, T's kx = 0 and kx = vdim/2 planes as given) and
    method 2 (even half-grid, the planes averaged first) on one T: each within
    the bar of float64, the same iteration count, and W of the two within the
    sum of their bars.  This is where a 3D C2R that read the two planes
    differently from FFTW would show."""
    T = recon_ref.sampling_density(family, N * pf, seed, p)
    ref = reference(N, pf, T, seed + 1000, {}, False)
    assert _stop_kind(ref["it"], ref["diffs"]) == stop
    label = f"{N}x{pf} {family} {seed}"
    W1, it1, d1 = check_weights(ref, N, pf, {}, 1, False, label)
    W2, it2, d2 = check_weights(ref, N, pf, {}, 2, True, label)
    assert it1 == it2
    rel = ((W1.double() - W2.double()).abs()[ref["inside"]] / ref["W"][ref["inside"]]).max()
    assert float(rel) <= 2 * BAR * ref["e32"]["W"]


# ------------------------------------------------------------------- options
OPTIONS = {
    "map": dict(fsc=FSC),
    "map_join_half": dict(fsc=FSC, join_half=True),
    "map_no_grid_corr": dict(fsc=FSC, grid_corr=False),
    "no_grid_corr": dict(grid_corr=False),
    "map_nfsc_6": dict(fsc=FSC[:6]),                   # shells past 5 take f = 0 -> 1e-3
    "map_fsc_edges": dict(fsc=FSC_EDGES),              # 1.5, -0.2, 1.0, 0.0
    "max_radius_half": dict(max_radius=-1),            # N / 2, filled in below
    "map_max_radius_6": dict(fsc=FSC, max_radius=6),   # the MAP band is shell 5 alone
    "map_max_radius_5": dict(fsc=FSC, max_radius=5),   # an empty MAP band
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("N", [16, 32])
def test_options_on_both_loops(N, opt):
    """(16, 2) runs the 3D-transform loop, (32, 2) the even one."""
    kw = dict(OPTIONS[opt])
    if kw.get("max_radius") == -1:
        kw["max_radius"] = N // 2
    ref = run_case(N, 2, "smooth", 1, kw=kw, exact_T=opt == "map_max_radius_5", tag=opt)
    if "fsc" in kw and opt != "map_max_radius_5":      # the MAP factor did act
        assert not torch.equal(ref["T_after"].float(), torch.clamp(ref["T"], min=1e-25))
