"""The round's last stage on the GPU (csrc/refresh.hip through
thunder_amd.reference): thx_ref_average, thx_projectee on both of its paths
(the pruned LDS passes and the fused pad + hipFFT fallback), thx_projectee2d.

The reference is tests/refresh_ref.py in float64.  The bound on every
projectee is max |gpu - ref| / max |ref| <= max(1e-5, 4 e32): 1e-5 is the
project's likelihood tolerance (the projectee is what the likelihood's
projections are gathered from), e32 the restatement's own error when it runs
in float32 on the same inputs, computed here and printed with the measured
error.  The shapes are the smallest at which each path can go wrong: vdim 32
is the smallest fft_lds pair with something to prune, N = 64 at pf 1 the
pruned path with nothing to prune, N = 24 a box that is no power of two.

Measured on an MI355X (every bound is 1e-5, since 4 e32 is below it): 3D
1.4e-7 .. 2.9e-7 on both paths with e32 0.7e-7 .. 2.7e-7; Fourier-space input
3.6e-7 .. 4.1e-7; 2D 1.5e-7 .. 1.9e-7; single-voxel closed forms 2.5e-7 ..
4.0e-7; the drop-in comparison through ops.project3d 1.3e-7 .. 1.7e-7; the
closed loop 1.9e-7.  Every test prints its figures."""
import functools

import numpy as np
import pytest
import torch

import refresh_ref as rr
from thunder_amd import ThxError, ops, reference, synth
from thunder_amd import expectation as ex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EDGE = 6


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the cached inputs are read-only


def corners(N):
    lo, hi = -N // 2, N // 2 - 1
    return [(lo, 0, 0), (0, lo, 0), (0, 0, lo), (hi, 0, 0), (0, hi, 0), (0, 0, hi), (lo, lo, lo),
            (hi, hi, hi), (lo, hi, 1), (1, 2, 0)]


@functools.lru_cache(maxsize=None)
def volume(N, seed=0):
    """Seeded Gaussian noise plus the corner voxels: every line carries signal."""
    v = np.random.default_rng(100 + N + seed).standard_normal((N, N, N)).astype(np.float32)
    for n, (i, j, k) in enumerate(corners(N)):
        v[k % N, j % N, i % N] = 4.0 + n
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def alpha(N):
    a = np.random.default_rng(200 + N).uniform(0, 1, (N, N, N)).astype(np.float32)
    a[0, 0, 0], a[0, 0, 1] = 0.0, 1.0
    a.setflags(write=False)
    return a


def mask_args(N, kind):
    return dict(mask_radius=N / 4 if kind == "radial" else None, mask=alpha(N) if kind == "alpha" else None)


@functools.lru_cache(maxsize=None)
def restated(N, pf, kind):
    """(float64 projectee, e32) of volume(N) under one mask kind; computed once."""
    kw = mask_args(N, kind)
    r64 = rr.projectee(volume(N), pf, edge=EDGE, **kw)
    r32 = rr.projectee(volume(N), pf, edge=EDGE, dtype=np.float32, **kw)
    e32 = float(np.max(np.abs(r32 - r64)) / np.max(np.abs(r64)))
    r64.setflags(write=False)
    return r64, e32


def gpu_projectee(N, pf, kind, method, src=None, **kw):
    a = mask_args(N, kind)
    return reference.refresh_projectee(T(volume(N)) if src is None else src, pf, a["mask_radius"],
                                       None if a["mask"] is None else T(a["mask"]), edge=EDGE,
                                       method=method, **kw)


def rel_err(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


SHAPES = [(16, 2, "pruned"), (32, 2, "pruned"), (64, 1, "pruned"), (24, 2, "fallback"),
          (32, 2, "fallback")]


@pytest.mark.parametrize("kind", ["radial", "alpha", "none"])
@pytest.mark.parametrize("N,pf,method", SHAPES)
def test_3d_against_restatement(N, pf, method, kind):
    ref, e32 = restated(N, pf, kind)
    got = gpu_projectee(N, pf, kind, method)
    vdim = pf * N
    assert got.shape == (vdim, vdim, vdim // 2 + 1) and ops._vol_dim(got) == vdim
    err = rel_err(got, ref)
    print(f"projectee N={N} pf={pf} {method} mask={kind}: gpu {err:.3e} e32 {e32:.3e} "
          f"bound {max(1e-5, 4 * e32):.3e}")
    assert err <= max(1e-5, 4 * e32)
    if kind == "radial" and N == 16:
        # all three branches of the soft mask occur, corners zeroed
        u = rr._norm_rl(N, 3, np.float64)
        assert (u < N / 4).any() and ((u >= N / 4) & (u <= N / 4 + EDGE)).any() and (u > N / 4 + EDGE).any()


def test_auto_serves_every_box():
    for N, pf in ((16, 2), (24, 2), (32, 2)):
        ref, e32 = restated(N, pf, "radial")
        assert rel_err(gpu_projectee(N, pf, "radial", "auto"), ref) <= max(1e-5, 4 * e32)
    with pytest.raises((ThxError, ValueError)):
        gpu_projectee(24, 2, "radial", "pruned")


@pytest.mark.parametrize("method", ["pruned", "fallback"])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_single_voxel_closed_form(method, interp):
    N, pf = 16, 2
    worst = 0.0
    for n, pos in enumerate(corners(N) + [(0, 0, 0)]):
        for mr in (None, N / 4):
            w = 1.0 + 0.5 * n
            src = np.zeros((N, N, N), np.float32)
            src[pos[2] % N, pos[1] % N, pos[0] % N] = w
            got = reference.refresh_projectee(T(src), pf, mr, edge=EDGE, interp=interp, method=method)
            ref = rr.single_voxel(N, pf, pos, w, mr, EDGE, interp)
            if np.max(np.abs(ref)) == 0:
                assert float(got.abs().max()) == 0.0
                continue
            worst = max(worst, rel_err(got, ref))
    print(f"single voxel {method} {interp}: worst {worst:.3e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("N,pf,method", [(16, 2, "pruned"), (32, 2, "pruned"), (24, 2, "fallback")])
def test_from_ft(N, pf, method):
    ref, e32 = restated(N, pf, "radial")
    ft = torch.fft.rfftn(T(volume(N))).to(torch.complex64).contiguous()
    keep = ft.clone()
    got = gpu_projectee(N, pf, "radial", method, src=ft)
    err = rel_err(got, ref)
    print(f"fromFT N={N} {method}: gpu {err:.3e} e32 {e32:.3e}")
    assert err <= max(1e-5, 4 * e32)
    assert torch.equal(ft, keep)                          # the source is not overwritten
    # the restatement's own Fourier-input branch agrees with its real-input one
    assert rel_err(rr.projectee(np.fft.rfftn(volume(N).astype(np.float64)), pf, N / 4, edge=EDGE),
                   ref) < 1e-12


def _halves(N, seed, lead=()):
    rng = np.random.default_rng(seed)
    shape = tuple(lead) + (N, N, N // 2 + 1)
    mk = lambda: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return mk(), mk()


@pytest.mark.parametrize("N", [16, 24])
def test_average_halves_bit_exact(N):
    A, B = _halves(N, 7)
    quad = rr._quad_ft(N, 3)
    for r in (0, 3, N // 2, -1):
        a, b = T(A), T(B)
        reference.average_halves(a, b, r)
        avg = (A + B) / np.complex64(2)
        sel = np.ones_like(quad, bool) if r < 0 else quad < r * r
        want_a, want_b = np.where(sel, avg, A), np.where(sel, avg, B)
        assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b), r
        ra, rb = rr.average(A, B, r, dtype=np.float32)
        assert np.array_equal(want_a, ra) and np.array_equal(want_b, rb)
        if r > 0:
            on = quad == r * r
            assert on.any() and np.array_equal(a.cpu().numpy()[on], A[on])
    a, b = T(A), T(B)
    reference.average_halves(a, b)                        # r None: the K > 1 branch
    assert np.array_equal(a.cpu().numpy(), (A + B) / np.complex64(2)) and torch.equal(a, b)
    a = T(A)
    reference.average_halves(a, None, 3)                  # no B: nothing to average
    assert np.array_equal(a.cpu().numpy(), A)


def test_average_halves_classes_and_2d():
    N = 16
    A, B = _halves(N, 8, lead=(3,))
    a, b = T(A), T(B)
    reference.average_halves(a, b, 4)
    for c in range(3):
        ra, rb = rr.average(A[c], B[c], 4, dtype=np.float32)
        assert np.array_equal(a[c].cpu().numpy(), ra) and np.array_equal(b[c].cpu().numpy(), rb)
    a, b = T(A[0]), T(B[0])                               # [nK = 16, N, N/2+1] images
    reference.average_halves(a, b, 4, mode2d=True)
    for c in (0, 5, 15):
        ra, rb = rr.average(A[0][c], B[0][c], 4, dims=2, dtype=np.float32)
        assert np.array_equal(a[c].cpu().numpy(), ra) and np.array_equal(b[c].cpu().numpy(), rb)


def test_low_pass_within_rounding():
    N = 16
    A, B = _halves(N, 9)
    thres, ew = 4.0 / N, 4.0 / N                          # solventFlatten: r / size, EDGE_WIDTH_FT / size
    a, b = T(A), T(B)
    reference.average_halves(a, b, 3, low_pass=(thres, ew))
    ra, rb = rr.average(A, B, 3)
    ra, rb = rr.low_pass(ra, thres, ew), rr.low_pass(rb, thres, ew)
    w = rr.low_pass(np.ones_like(ra), thres, ew).real
    assert (w == 1).any() and (w == 0).any() and ((w > 0) & (w < 1)).any()
    for g, r_ in ((a, ra), (b, rb)):
        g = g.cpu().numpy()
        assert np.max(np.abs(g - r_)) <= 1e-6 * np.max(np.abs(r_))
        assert np.all(g[w == 0] == 0)
    a = T(A)
    reference.average_halves(a, None, low_pass=(thres, ew))   # the filter alone
    assert np.max(np.abs(a.cpu().numpy() - rr.low_pass(A, thres, ew))) <= 1e-6 * np.max(np.abs(A))


@pytest.mark.parametrize("N,pf,method", [(32, 2, "pruned"), (32, 2, "fallback"), (24, 2, "fallback")])
def test_run_to_run_determinism(N, pf, method):
    for kind in ("radial", "alpha"):
        a = gpu_projectee(N, pf, kind, method).clone()
        b = gpu_projectee(N, pf, kind, method)
        assert torch.equal(a.view(torch.float32), b.view(torch.float32))
    ft = torch.fft.rfftn(T(volume(N))).to(torch.complex64).contiguous()
    a = gpu_projectee(N, pf, "radial", method, src=ft).clone()
    b = gpu_projectee(N, pf, "radial", method, src=ft)
    assert torch.equal(a.view(torch.float32), b.view(torch.float32))


@pytest.mark.parametrize("method", ["pruned", "fallback"])
def test_scale_makes_a_drop_in_projectee(method):
    """scale = N^-1.5, no mask: synth.projectee of the same volume but for the
    grid correction.  With the correction taken out of synth's input the two
    agree through ops.project3d at rU = N/2 - 2."""
    N, pf = 32, 2
    vol = synth.blob_volume(N, n_blobs=8, seed=4).numpy().astype(np.float64)     # centred at N/2
    wrapped = np.fft.ifftshift(vol)                                               # origin at [0, 0, 0]
    tik = rr.kernel_rl(rr._norm_rl(N, 3, np.float64) / (pf * pf * N))             # wrapped layout
    got = reference.refresh_projectee(T(wrapped.astype(np.float32)), pf, scale=N ** -1.5, method=method)
    want = synth.projectee(torch.as_tensor(np.fft.fftshift(wrapped / tik).astype(np.float32)), pf).to(DEV)
    px = ops.PixelSet(N, pf, N // 2 - 2, 0, device=DEV)
    mat = ops.rotmat(T(synth.uniform_quaternions(16, np.random.default_rng(5))))
    pg, pw = ops.project3d(got, mat, px), ops.project3d(want, mat, px)
    err = float((pg - pw).abs().max() / pw.abs().max())
    print(f"scale / drop-in {method}: {err:.3e}")
    assert err <= 1e-5
    # and without taking it out they differ by the correction, which is not small
    plain = synth.projectee(torch.as_tensor(vol.astype(np.float32)), pf).to(DEV)
    assert float((got - plain).abs().max() / plain.abs().max()) > 1e-3


@pytest.mark.parametrize("N", [16, 24])
def test_2d_against_restatement(N):
    nK, pf = 3, 2
    imgs = np.stack([volume(N, seed=c)[c] for c in range(nK)])
    for mr in (N / 4, None):
        r64 = rr.projectee2d(imgs, pf, mr, EDGE)
        r32 = rr.projectee2d(imgs, pf, mr, EDGE, dtype=np.float32)
        e32 = float(np.max(np.abs(r32 - r64)) / np.max(np.abs(r64)))
        got = reference.refresh_projectee(T(imgs), pf, mr, edge=EDGE, mode2d=True)
        assert got.shape == (nK, pf * N, pf * N // 2 + 1) and ops._img2d_dim(got) == pf * N
        err = rel_err(got, r64)
        print(f"2D N={N} mask={mr}: gpu {err:.3e} e32 {e32:.3e}")
        assert err <= max(1e-5, 4 * e32)
        ft = torch.fft.rfftn(T(imgs), dim=(-2, -1)).to(torch.complex64).contiguous()
        got = reference.refresh_projectee(ft, pf, mr, edge=EDGE, mode2d=True)
        assert rel_err(got, r64) <= max(1e-5, 4 * e32)
    # closed forms, 2D: the wrap corner unmasked, an edge pixel under the mask
    for pos, mr in (((-N // 2, N // 2 - 1), None), ((-N // 4, 2), N / 4)):
        src = np.zeros((1, N, N), np.float32)
        src[0, pos[1] % N, pos[0] % N] = 2.0
        got = reference.refresh_projectee(T(src), pf, mr, edge=EDGE, mode2d=True)[0]
        assert rel_err(got, rr.single_voxel(N, pf, pos, 2.0, mr, EDGE)) <= 1e-5


def test_2d_rejects_a_provided_mask():
    N = 16
    with pytest.raises(ValueError):
        reference.refresh_projectee(T(np.zeros((3, N, N), np.float32)), 2, mask=T(alpha(N)), mode2d=True)
    from thunder_amd._lib import lib
    src = T(np.zeros((3, N, N), np.float32))
    dst = torch.empty(3, 2 * N, N + 1, dtype=torch.complex64, device=DEV)
    ws = ops.workspace(lib().thx_projectee2d_workspace(N, 2, 3, 0), DEV)
    st = lib().thx_projectee2d(ops._ptr(src), 0, 3, N, 2, 0.0, 6.0, ops._ptr(T(alpha(N))), 0, 1.0,
                               ops._ptr(dst), ops._ptr(ws), ws.numel(), ops._stream(DEV))
    assert st == 1


def test_class_axis_and_out():
    N, pf = 16, 2
    ref, e32 = restated(N, pf, "radial")
    stack = T(np.stack([volume(N), 2 * volume(N)]))
    out = torch.empty(2, pf * N, pf * N, pf * N // 2 + 1, dtype=torch.complex64, device=DEV)
    got = reference.refresh_projectee(stack, pf, N / 4, edge=EDGE, out=out)
    assert got is out
    assert rel_err(got[0], ref) <= max(1e-5, 4 * e32) and rel_err(got[1], 2 * ref) <= max(1e-5, 4 * e32)


@pytest.fixture(scope="module")
def closed_loop():
    """blob -> projectee -> noise-free projections at known poses -> insert ->
    reconstruct -> the map whose projectee the next round needs."""
    N, pf = 32, 2
    vol = synth.projectee(synth.blob_volume(N, n_blobs=10, seed=6, device=DEV), pf)
    px = ops.PixelSet(N, pf, N // 2 - 2, 0, device=DEV)
    rng = np.random.default_rng(12)
    n = 300
    quat = T(synth.uniform_quaternions(n, rng))
    dat = ops.project3d(vol, ops.rotmat(quat), px)
    hm = ops.HalfMap(pf * N, DEV)
    ops.insert3d(hm, dat, torch.ones(n, px.n, device=DEV), quat.reshape(n, 1, 4).contiguous(),
                 torch.zeros(n, 1, 2, dtype=torch.float64, device=DEV),
                 torch.zeros(n, 2, dtype=torch.float64, device=DEV), torch.ones(n, device=DEV), px)
    dst, dft, _, _ = ops.reconstruct(hm, N, pf)
    return dict(N=N, pf=pf, px=px, vol=vol, dst=dst, dft=dft)


@pytest.mark.parametrize("method", ["pruned", "fallback"])
def test_loop_closure(closed_loop, method):
    c = closed_loop
    N, pf, px = c["N"], c["pf"], c["px"]
    mr, sc = N / 2 - 4, N ** -1.5
    dst = c["dst"].cpu().numpy()
    assert np.all(np.isfinite(dst)) and np.abs(dst).max() > 0
    r64 = rr.projectee(dst, pf, mr, edge=EDGE, scale=sc)
    r32 = rr.projectee(dst, pf, mr, edge=EDGE, scale=sc, dtype=np.float32)
    e32 = float(np.max(np.abs(r32 - r64)) / np.max(np.abs(r64)))
    got = reference.refresh_projectee(c["dst"], pf, mr, edge=EDGE, scale=sc, method=method)
    mat = ops.rotmat(T(synth.uniform_quaternions(32, np.random.default_rng(13))))
    pg = ops.project3d(got, mat, px)
    pr = ops.project3d(T(r64.astype(np.complex64)), mat, px)
    err = float((pg - pr).abs().max() / pr.abs().max())
    print(f"loop closure {method}: projections {err:.3e} e32 {e32:.3e}")
    assert err <= max(1e-5, 4 * e32)
    # the reconstruction's transform (dstFT) gives the same projectee
    got_ft = reference.refresh_projectee(c["dft"], pf, mr, edge=EDGE, scale=sc, method=method)
    assert rel_err(got_ft, r64) <= max(1e-5, 4 * e32)


def test_driver_takes_the_result(closed_loop):
    c = closed_loop
    N, pf = c["N"], c["pf"]
    vol = reference.refresh_projectee(c["dst"], pf, N / 2 - 4, edge=EDGE, scale=N ** -1.5)
    px = ops.PixelSet(N, pf, 8, 1, device=DEV)
    gset = synth.global_sample_set(300, seed=14)
    rng = np.random.default_rng(15)
    n = 8
    qtrue = T(gset[0][rng.integers(0, 300, n)])
    ctf = ops.ctf(T(synth.ctf_attrs(n, seed=16)), px)
    sigl = ctf * ops.project3d(vol, ops.rotmat(qtrue), px)
    dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=20.0, seed=17)
    e = ex.Expectation(vol, px, gset, n_phase=2, seed=5)
    quat, trans, pR, pT, score = e.run(dat, ctf, sig)[:5]
    assert quat.shape[0] == n and torch.isfinite(quat).all() and torch.isfinite(trans).all()
    assert torch.isfinite(score).all()
