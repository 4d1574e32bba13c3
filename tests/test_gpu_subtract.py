"""Signal subtraction on the GPU (csrc/subtract.hip, thunder_amd/subtract.py)
against the float64 restatement of tests/subtract_ref.py: diffFT, modelFT,
diffRL, the copies' quaternions and the shift of saveSubtract
(src/Optimiser.cpp:8418-8537, 8295-8361), and the region centre
(src/Image/ImageFunctions.cpp:37-62).

Fourier-space cases write ori directly in Fourier space: the model at the true
pose plus independent complex noise on EVERY stored pixel -- column 0 below the
axis included, so it is deliberately not Hermitian-consistent -- and stronger
garbage outside the disc, which has to pass through with the phase only.
Real-space cases take ori = rfft2 of a real image and volumes of real maps.

The bound holds per output plane: max |gpu - ref64| / max |ori_l| <=
max(1e-5, 4 e32), the rule of test_gpu_noise.py: 1e-5 is the project's
likelihood tolerance, e32 the same metric for the restatement run in numpy
float32 against its float64 run on the same inputs, computed here and printed.
Real-space planes are normalised by the real-space input, max |irfft2(ori_l)|.
"""
import types

import numpy as np
import pytest
import torch

import subtract_ref
from thunder_amd import io, ops, subtract, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PF = 2
N_IMG = 7
CLS = np.array([0, 1, 1, 0, 1, 0, 0], np.int32)
DF = np.array([1.0, 1.02, 1.0, 0.97, 1.0, 1.0, 1.01])
SHAPES = [(32, 15), (64, 31), (32, 10)]      # r = maxR twice; a wide pass-through ring
SYMS = [None, "C2", "D2"]                    # nSym 0, 1, 3


def T_(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


_vols = {}


def volumes(N):
    if N not in _vols:
        _vols[N] = np.stack([synth.projectee(synth.blob_volume(N, n_blobs=30, seed=s), PF).numpy()
                             for s in (1, 2)])
    return _vols[N]


def sym_matrices(sym):
    return None if sym is None else ops.symmetry(sym)[0]


def _noise(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


_cases = {}


def make_case(orc, N, r, sym, hermitian=False, noise_free=False, seed=3):
    """one stack with its float64 reference and float32 error"""
    key = (N, r, sym, hermitian, noise_free, seed)
    if key in _cases:
        return _cases[key]
    vdim = N * PF
    vols = volumes(N)
    rng = np.random.default_rng(seed + N + r)
    c = types.SimpleNamespace(N=N, r=r, vdim=vdim, vols=vols, sym=sym, symR=sym_matrices(sym))
    c.attr = synth.ctf_attrs(N_IMG, seed=seed + 5)
    c.quat = synth.uniform_quaternions(N_IMG, rng)
    c.trans = rng.standard_normal((N_IMG, 2)) * 2
    c.off = rng.standard_normal((N_IMG, 2)) * 1.5
    c.centre = np.array([1.5, -2.25, 0.75]) * (N / 32)
    nc = N // 2 + 1
    # the signal: the float64 model of copy 0 at the true poses
    zero = np.zeros((N_IMG, N, nc), np.complex128)
    sig = subtract_ref.subtract(orc, vols, vdim, PF, zero, c.attr, c.quat, c.trans, r, N, c.off, DF,
                                CLS).modelFT[0]
    gi, gj = subtract_ref.grid(N)
    in_disc = (gi * gi + gj * gj < r * r).reshape(N, nc)
    amp = np.sqrt(np.mean(np.abs(sig[:, in_disc]) ** 2))
    if noise_free:
        ori = sig
    elif hermitian:
        img = np.fft.irfft2(sig, s=(N, N)) + amp / N * rng.standard_normal((N_IMG, N, N))
        ori = np.fft.rfft2(img)
    else:
        ori = sig + np.where(in_disc, amp, 3 * amp) * _noise(rng, sig.shape)
    c.ori = ori.astype(np.complex64)
    c.scale = np.abs(c.ori).reshape(N_IMG, -1).max(1)                      # max |ori_l|
    c.scale_rl = np.abs(np.fft.irfft2(c.ori.astype(np.complex128), s=(N, N))).reshape(
        N_IMG, -1).max(1)
    args = (orc, vols, vdim, PF, c.ori, c.attr, c.quat, c.trans, r, N, c.off, DF, CLS, c.symR,
            c.centre)
    c.ref = subtract_ref.subtract(*args)
    r32 = subtract_ref.subtract(*args, dtype=np.float32)
    c.e32 = {k: plane_error(getattr(r32, k), getattr(c.ref, k),
                            c.scale_rl if k == "diffRL" else c.scale)
             for k in ("diffFT", "modelFT", "diffRL")}
    _cases[key] = c
    return c


def plane_error(got, ref, scale):
    """the worst plane of [copies, n, ...]: max |got - ref| / scale[l]"""
    d = np.abs(np.asarray(got) - ref).reshape(ref.shape[0], ref.shape[1], -1).max(2)
    return float((d / scale[None, :]).max())


def gpu_run(c, cls=CLS, **kw):
    kw.setdefault("model", True)
    return subtract.subtract(T_(c.vols), T_(c.ori), T_(c.attr), T_(c.quat), T_(c.trans), c.r, PF,
                             T_(c.off), T_(DF), T_(cls), c.symR, T_(c.centre), **kw)


def check_fourier(c, o, what):
    for k in ("diffFT", "modelFT"):
        err = plane_error(getattr(o, k).cpu().numpy(), getattr(c.ref, k), c.scale)
        bound = max(1e-5, 4 * c.e32[k])
        print(f"{what} {k}: gpu {err:.3e} e32 {c.e32[k]:.3e} bound {bound:.3e}")
        assert err <= bound, k


def check_poses(c, o):
    q = o.quat.cpu().numpy()
    assert q.shape == c.ref.quat.shape
    for s in range(q.shape[0]):
        for l in range(N_IMG):
            assert np.allclose(subtract_ref.quat_matrix(q[s, l]),
                               subtract_ref.quat_matrix(c.ref.quat[s, l]), rtol=0, atol=1e-12)
    assert np.allclose(o.shift.cpu().numpy(), c.ref.shift, rtol=0, atol=1e-12)


@pytest.mark.parametrize("sym", SYMS, ids=["c1", "c2", "d2"])
@pytest.mark.parametrize("N,r", SHAPES)
def test_fourier_outputs(orc, N, r, sym):
    c = make_case(orc, N, r, sym)
    o = gpu_run(c, real=False)
    assert o.diffRL is None and o.n_sym == (0 if c.symR is None else len(c.symR))
    assert o.diffFT.shape == (1 + o.n_sym, N_IMG, N, N // 2 + 1)
    check_fourier(c, o, f"N={N} r={r} {sym}")
    check_poses(c, o)
    # the domain: the model is exactly 0 outside i^2 + j^2 < r^2 (rows j = +-r
    # and the pixels at |.| = r included), and set wherever the reference sets it
    i, j = subtract_ref.grid(N)
    inside = (i * i + j * j < r * r).reshape(N, N // 2 + 1)
    m = o.modelFT.cpu().numpy()
    assert np.all(m[..., ~inside] == 0) and np.all(c.ref.modelFT[..., ~inside] == 0)
    assert np.mean(m[..., inside] != 0) > 0.999
    # outside the disc, the Nyquist row and column included, ori gets the phase
    # only: its modulus stays (1e-4: a unit phasor from the FP32 sin / cos;
    # anything subtracted there would move it by the garbage's own size)
    d = o.diffFT.cpu().numpy()
    ring = ~inside
    assert ring[N // 2].all() and ring[:, N // 2].all()
    assert np.allclose(np.abs(d[..., ring]), np.abs(c.ori[None][..., ring]), rtol=1e-4, atol=0)
    again = gpu_run(c, real=False)
    for k in ("diffFT", "modelFT", "quat", "shift"):
        assert torch.equal(getattr(o, k), getattr(again, k)), k          # bit-identical runs


@pytest.mark.parametrize("sym", ["I1", "C67"])
def test_many_copies(orc, sym):
    """I1: 60 copies in the LDS table; C67: 67 copies, more than the table
    holds at a time"""
    c = make_case(orc, 32, 10, sym)
    assert len(c.symR) == (59 if sym == "I1" else 66)
    o = gpu_run(c, real=False)
    check_fourier(c, o, f"N=32 r=10 {sym}")
    check_poses(c, o)


@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("N,r", SHAPES)
def test_real_space(orc, N, r, centred):
    c = make_case(orc, N, r, "D2", hermitian=True)
    o = gpu_run(c, real=True, centred=centred)
    check_fourier(c, o, f"N={N} r={r} hermitian")          # diffFT survives the C2R
    ref = subtract_ref.centred(c.ref.diffRL) if centred else c.ref.diffRL
    err = plane_error(o.diffRL.cpu().numpy(), ref, c.scale_rl)
    bound = max(1e-5, 4 * c.e32["diffRL"])
    print(f"N={N} r={r} centred={centred} diffRL: gpu {err:.3e} e32 {c.e32['diffRL']:.3e} "
          f"bound {bound:.3e}")
    assert err <= bound
    # straight from the workspace, without diffFT
    only = gpu_run(c, real=True, centred=centred, ft=False, model=False)
    assert only.diffFT is None and only.modelFT is None
    assert torch.equal(only.diffRL, o.diffRL)
    assert torch.equal(gpu_run(c, real=True, centred=centred).diffRL, o.diffRL)


def test_defaults(orc):
    """each optional input NULL: offS 0, dF 1, class 0, no symmetry, centre 0"""
    c = make_case(orc, 32, 10, None)
    ref = subtract_ref.subtract(orc, c.vols, c.vdim, PF, c.ori, c.attr, c.quat, c.trans, c.r, 32)
    d = subtract.subtract(T_(c.vols[0]), T_(c.ori), T_(c.attr), T_(c.quat), T_(c.trans), c.r, PF,
                          real=False, model=True)
    bound = max(1e-5, 4 * c.e32["diffFT"])
    assert plane_error(d.diffFT.cpu().numpy(), ref.diffFT, c.scale) <= bound
    assert plane_error(d.modelFT.cpu().numpy(), ref.modelFT, c.scale) <= bound
    e = subtract.subtract(T_(c.vols), T_(c.ori), T_(c.attr), T_(c.quat), T_(c.trans), c.r, PF,
                          T_(np.zeros((N_IMG, 2))), T_(np.ones(N_IMG)),
                          T_(np.zeros(N_IMG, np.int32)), np.zeros((0, 3, 3)), T_(np.zeros(3)),
                          real=False, model=True)
    for k in ("diffFT", "modelFT", "quat", "shift"):
        assert torch.equal(getattr(d, k), getattr(e, k)), k
    # one NULL at a time against the full call's restatement inputs
    full = gpu_run(c, real=False)
    no_centre = subtract.subtract(T_(c.vols), T_(c.ori), T_(c.attr), T_(c.quat), T_(c.trans), c.r,
                                  PF, T_(c.off), T_(DF), T_(CLS), None, None, real=False,
                                  model=True)
    assert torch.equal(no_centre.modelFT, full.modelFT)        # the centre moves diff only
    r0 = subtract_ref.subtract(orc, c.vols, c.vdim, PF, c.ori, c.attr, c.quat, c.trans, c.r, 32,
                               c.off, DF, CLS)
    assert plane_error(no_centre.diffFT.cpu().numpy(), r0.diffFT, c.scale) <= bound


def test_roll_identity(orc):
    """a zero projectee, the identity pose and -t + offS - centre = (3, -2):
    the real-space output is the input image rolled by (3, -2)"""
    N, r = 32, 15
    rng = np.random.default_rng(11)
    img = rng.standard_normal((N_IMG, N, N))
    ori = np.fft.rfft2(img).astype(np.complex64)
    img = np.fft.irfft2(ori.astype(np.complex128), s=(N, N))       # what complex64 holds
    quat = np.tile([1.0, 0, 0, 0], (N_IMG, 1))
    centre = np.array([-1.0, 0.5, 2.0])
    off = rng.standard_normal((N_IMG, 2))
    trans = off - centre[:2] - np.array([3.0, -2.0])
    vols = torch.zeros(1, N * PF, N * PF, N * PF // 2 + 1, dtype=torch.complex64, device=DEV)
    o = subtract.subtract(vols, T_(ori), T_(synth.ctf_attrs(N_IMG)), T_(quat), T_(trans), r, PF,
                          T_(off), centre=T_(centre), centred=False)
    want = np.roll(img, (-2, 3), axis=(1, 2))
    scale = np.abs(img).reshape(N_IMG, -1).max(1)
    # the float32 restatement's own error on this input
    e32 = plane_error(subtract_ref.subtract(orc, vols.cpu().numpy(), N * PF, PF, ori,
                                            synth.ctf_attrs(N_IMG), quat, trans, r, N, off,
                                            centre=centre, dtype=np.float32).diffRL,
                      want[None], scale)
    err = plane_error(o.diffRL.cpu().numpy(), want[None], scale)
    print(f"roll identity: gpu {err:.3e} e32 {e32:.3e}")
    assert err <= max(1e-5, 4 * e32)


def test_noise_free_difference_vanishes(orc):
    """images that are the model itself: |diff| is within the bound of 0 on the
    disc -- a wrong CTF or phase sign would leave the whole signal"""
    c = make_case(orc, 32, 15, None, noise_free=True)
    o = gpu_run(c, real=False)
    d = np.abs(o.diffFT.cpu().numpy()[0]).reshape(N_IMG, -1).max(1) / c.scale
    bound = max(1e-5, 4 * c.e32["diffFT"])
    print("noise-free: worst |diff| / max |ori|", float(d.max()), "bound", bound)
    assert np.all(d <= bound)
    assert np.abs(o.modelFT.cpu().numpy()[0]).max() > 0.5 * c.scale.max()


def test_class_out_of_range(orc):
    c = make_case(orc, 32, 10, "C2", hermitian=True)
    good = gpu_run(c, real=True)
    bad = CLS.copy()
    bad[2] = 2                       # outside the two projectees: NaN, no gather
    b = gpu_run(c, cls=bad, real=True)
    rest = [0, 1, 3, 4, 5, 6]
    for k in ("diffFT", "modelFT", "diffRL", "quat"):
        g, x = getattr(good, k), getattr(b, k)
        assert torch.isnan(torch.view_as_real(x[:, 2]) if x.is_complex() else x[:, 2]).all(), k
        assert torch.equal(x[:, rest], g[:, rest]), k
    assert torch.isnan(b.shift[2]).all() and torch.equal(b.shift[rest], good.shift[rest])


def soft_mask(N, c, rad, edge):
    co = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(np.float64)
    k, j, i = np.meshgrid(co, co, co, indexing="ij")
    d = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2)
    return np.exp(-np.maximum(d - rad, 0) ** 2 / (2 * edge ** 2)).astype(np.float32)


@pytest.mark.parametrize("N", [16, 32])          # one block; several blocks
def test_region_centroid(N):
    m = soft_mask(N, (2.0 * N / 16, -1.5 * N / 16, 3.0 * N / 16), N / 8, N / 12)
    ref = subtract_ref.region_centroid(m)
    a = subtract.region_centroid(T_(m))
    b = subtract.region_centroid(T_(m))
    assert torch.equal(a, b)                                         # bit-identical
    got = a.cpu().numpy()
    print(f"centroid N={N}: {got} ref {ref}")
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref))


def test_save_subtract(orc, tmp_path):
    """end to end at box 32 with C2, in chunks of 3 images: the stack on disk
    is the one-call diffRL, the table has one row per (image, copy)"""
    c = make_case(orc, 32, 15, "C2", hermitian=True)
    st = types.SimpleNamespace(oriFT=T_(c.ori), attr=T_(c.attr), pixel_size=1.32)
    prefix = str(tmp_path) + "/"
    group = np.arange(N_IMG) % 3
    sp, tp, shift = subtract.save_subtract(st, T_(c.vols), T_(c.quat), T_(c.trans), c.r, prefix, PF,
                                           T_(c.off), T_(DF), T_(CLS), "C2", T_(c.centre),
                                           group=group, rank=1, chunk=3)
    one = gpu_run(c, real=True, model=False)
    h, data = io.read_mrc(sp)
    assert (h.nz, h.ny, h.nx) == (2 * N_IMG, 32, 32)
    assert np.array_equal(np.asarray(data), one.diffRL.cpu().numpy().reshape(-1, 32, 32))
    assert torch.equal(shift, one.shift)
    t = io.read_thu(tp)
    assert len(t["particlePath"]) == 2 * N_IMG
    q = one.quat.cpu().numpy()
    for row, (l, s) in enumerate((l, s) for l in range(N_IMG) for s in range(2)):
        assert t["particlePath"][row] == "%012d@Subtract_Rank_000001.mrcs" % (l + N_IMG * s + 1)
        assert np.allclose([t[f"quat{k}"][row] for k in range(4)], q[s, l], atol=1e-9)
        assert t["transX"][row] == 0 and t["transY"][row] == 0
        assert t["classID"][row] == CLS[l] and t["groupID"][row] == group[l]
        assert t["defocusFactor"][row] == pytest.approx(DF[l], abs=1e-9)
