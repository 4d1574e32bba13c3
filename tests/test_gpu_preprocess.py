"""The image preprocessing kernels of thunder_amd/csrc/preprocess.hip
(thx_img_stats, thx_img_finish, thx_remask, thx_img_gather, thx_ctf_image, and
thx_GCTFinit over the last) against float64 references at their edge shapes:
the numpy restatement oracle/preprocess.py, the Philox restatement
tests/philox_ref.py for the noise background, and the C restatement's CTF
(oracle/oracle.py) on a hand-made list of every half-complex pixel.

Comparator.  A half-complex device result is brought back to real space with
numpy's float64 irfft2 and compared pixel by pixel with the float64 masked
image, per image, as max |got - ref| <= TOL x max |ref| (opp.rl_error).  A
mask weight wrong by 1e-3 at one edge pixel is 1.5e-4 there and invisible to a
Fourier-space bound (tests/test_ingest.py::
test_real_space_comparison_sees_one_wrong_mask_weight).

Measured on an MI355X, the worst image of each shape, max |got - ref| /
max |ref| of the inputs of this module (finish: the larger of imgFT and oriFT;
remask: the larger of the masked and the arbitrary input):

    N   r     ew   images   finish, zero   finish, noise   remask
    8   2.5   2.0       7   8.31e-08       -               1.94e-07
    16  5.0   2.0       7   1.43e-07       -               1.72e-07
    20  6.3   3.0       7   1.27e-07       -               2.06e-07
    24  5.0   5.0       7   1.54e-07       1.54e-07        2.26e-07
    36  11.7  6.0       7   1.47e-07       -               2.23e-07
    32  10.5  6.0     513   2.50e-07       2.57e-07        2.93e-07
    36  11.7  6.0     410   -              -               3.41e-07

(a float32 rfft2 on the CPU loses 0.6 to 1.7e-07 at the same inputs.)  TOL is
4 x the worst entry, 3.412e-07: 1.365e-06, under the 1e-5 (opp.RL_TOL_MAX) that
keeps it 10 times below what a 1e-3 error of one mask weight produces.  The
normalised images of thx_img_stats came out bit-equal to the restatement's at
every shape, and the CTF grids within 3.9e-06 of the oracle's (bound 5e-5).

Which test reaches what:
  centred = 0 and 1 ................ test_stats_both_layouts (every shape)
  zeroMask = 1, ori / oriFT given .. test_finish_zero_mask
  ori = oriFT = NULL ............... test_finish_zero_mask (keep_ori=False)
  zeroMask = 0 (Philox noise) ...... test_finish_noise_mask
  nImg = 513 > FFT_BATCH = 512 (second batch, tail plan of batch 1):
      fft_forward .................. test_finish_zero_mask, test_finish_noise_mask
      thx_remask ................... test_remask
  second trip of a grid-stride loop (more than 2048 x 256 elements):
      k_img_mask_scale ............. test_finish_zero_mask / _noise_mask (513 x 1024)
      k_scale_mask_rl .............. test_remask_wraps_the_grid (410 x 1296: the
                                     kernel runs once per batch of at most 512
                                     images, and 512 x 32 x 32 is exactly one
                                     trip, so the 513-image shape does not wrap it)
      k_img_gather ................. test_gather_wraps_the_grid (1000 x 544)
      k_ctf_image .................. test_ctf_image_many_images (4000 x 144)
  N not a power of two ............. the shapes 20, 24, 36
  N^2 < 256 (idle threads) ......... the shape 8
  lattice points on r and r + ew ... the shapes 16 and 24
  c = 0 and c = 1 background ....... test_stats_degenerate_background
  Nyquist column, row jj = N / 2 ... test_ctf_image_whole_grid, test_gctfinit_whole_grid
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import philox_ref
from oracle import preprocess as opp
from oracle.oracle import PixelSet
from thunder_amd import ingest
from thunder_amd._lib import check, lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

WORST_MEASURED = 3.412e-7
TOL = 4 * WORST_MEASURED
assert TOL <= opp.RL_TOL_MAX

# (N, r, ew, images)
SHAPES = [(8, 2.5, 2.0, 7), (16, 5.0, 2.0, 7), (20, 6.3, 3.0, 7), (24, 5.0, 5.0, 7),
          (36, 11.7, 6.0, 7), (32, 10.5, 6.0, 513)]
NOISE_SHAPES = [SHAPES[3], SHAPES[5]]
IDS = lambda s: f"N{s[0]}-r{s[1]}-ew{s[2]}-n{s[3]}"


def T(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)          # a copy: case() is read-only


def H(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(N, r, ew, n):
    """A synthetic stack in the corner-origin layout (a smooth blob plus
    noise, an offset and a gain per image) and its float64 references, made
    once per shape and never written to."""
    rng = np.random.default_rng(1000 * N + n)
    i, j = opp.rl_coords(N)
    blob = np.exp(-(i ** 2 + j ** 2) / (2 * (N / 6.0) ** 2)) * (1 + 0.3 * np.cos(4 * np.pi * i / N))
    gain, off = rng.uniform(0.5, 3.0, (n, 1, 1)), rng.uniform(-5.0, 5.0, (n, 1, 1))
    img = (gain * (3 * blob + 0.5 * rng.standard_normal((n, N, N))) + off).astype(np.float32)
    ref = [opp.stats_and_normalise(x, r) for x in img]
    rn = np.stack([x[0] for x in ref])
    rs = np.stack([x[1] for x in ref])
    std_n = float(rs[:, 2].mean())
    u = np.hypot(i, j).astype(np.float32)
    c = dict(img=img, rn=rn, rs=rs, std_n=std_n, u=u,
             masked=opp.masked_image(rn, r, std_n, ew), ori=rn.astype(np.float64) / std_n)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    # the regions every shape must have: background, inside, edge, beyond the edge
    assert (u * u > r * r).any() and (u < r).any() and ((u > r) & (u < r + ew)).any() \
        and (u > r + ew).any()
    return c


def rl_check(what, shape, ft, ref):
    e = opp.rl_error(H(ft), ref)
    print(f"MEASURED {what} {IDS(shape)} worst {e.max():.3e} (image {int(e.argmax())})")
    assert np.all(e <= TOL), (what, shape, float(e.max()), int(e.argmax()))


# ---------------------------------------------------------------- thx_img_stats
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stats_both_layouts(shape):
    """substractBgImg + statImg's terms for the stack given in the corner-origin
    layout (centred = 0) and rolled by N / 2 as on disk (centred = 1): the two
    agree bit for bit and with the restatement; at the lattice-point radii the
    pixels on r are neither background nor inside."""
    N, r, ew, n = shape
    c = case(*shape)
    assert np.array_equal(opp.load(np.roll(c["img"], (N // 2, N // 2), axis=(1, 2))), c["img"])
    n0, s0 = ingest.image_stats(T(c["img"]), False, r)
    n1, s1 = ingest.image_stats(T(np.roll(c["img"], (N // 2, N // 2), axis=(1, 2))), True, r)
    assert torch.equal(n0, n1) and torch.equal(s0, s1)
    e = np.abs(H(n0) - c["rn"]).max(axis=(1, 2)) / np.abs(c["rn"]).max(axis=(1, 2))
    print(f"MEASURED stats image {IDS(shape)} worst {e.max():.3e}")
    assert np.all(e <= 1e-5)
    assert np.allclose(H(s0), c["rs"], rtol=1e-5, atol=1e-6)
    # the per-image offsets and gains came through: bgMean and bgSd differ between images
    assert np.ptp(c["rs"][:, 0]) > 1 and np.ptp(c["rs"][:, 1]) > 0.1


@pytest.mark.parametrize("r,nbg", [(12.0, 0), (11.0, 1)])
def test_stats_degenerate_background(r, nbg):
    """N = 16: r = 12 leaves no pixel outside the radius, r = 11 exactly one,
    the corner (-8, -8).  The reference divides by zero; the kernel takes
    bgSd = 1, bgMean = 0 or that pixel's value, reports bgStddev(0) = 0, and
    the image comes out finite as x - bgMean."""
    N, n = 16, 5
    img = case(16, 5.0, 2.0, 7)["img"][:n]
    i, j = opp.rl_coords(N)
    bg = i.astype(np.float64) ** 2 + j.astype(np.float64) ** 2 > r * r
    assert bg.sum() == nbg and (nbg == 0 or bg[N // 2, N // 2])
    mean = img[:, N // 2, N // 2] if nbg else np.zeros(n, np.float32)
    want = img - mean[:, None, None]
    for centred in (False, True):
        x = np.roll(img, (N // 2, N // 2), axis=(1, 2)) if centred else img
        out, st = (H(t) for t in ingest.image_stats(T(x), centred, r))
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(st))
        assert np.array_equal(out, want)
        assert np.array_equal(st[:, 0], mean) and np.all(st[:, 1] == 1) and np.all(st[:, 2] == 0)
        o = want.astype(np.float64)
        a0 = np.sqrt((o ** 2).sum(axis=(1, 2)) / (N * N - 1))
        cm = o[:, np.hypot(i, j) < r].mean(axis=1)
        assert np.allclose(st[:, 3], a0, rtol=1e-5, atol=1e-6)
        assert np.allclose(st[:, 4], cm, rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------- thx_img_finish
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_finish_zero_mask(shape):
    N, r, ew, n = shape
    c = case(*shape)
    ft, oft = ingest.finish(T(c["rn"]), r, c["std_n"], zero_mask=True, keep_ori=True, edge=ew)
    rl_check("finish-zero imgFT", shape, ft, c["masked"])
    rl_check("finish-zero oriFT", shape, oft, c["ori"])
    ft2, none = ingest.finish(T(c["rn"]), r, c["std_n"], zero_mask=True, keep_ori=False, edge=ew)
    assert none is None and torch.equal(torch.view_as_real(ft2), torch.view_as_real(ft))


@pytest.mark.parametrize("shape", NOISE_SHAPES, ids=IDS)
def test_finish_noise_mask(shape):
    """zeroMask = 0: the background is N(0, stdN) per pixel from the Philox
    stream (q >> 32, q, 'mask') of flat pixel index q.  Against the
    restatement fed philox_ref's draws; a seed fixes the result; another seed
    changes every pixel beyond r and none within it (on r itself the
    background's weight is 0: Mask.cpp's w = 0.5 - 0.5 cos 0); the unmasked
    copy does not depend on the mask."""
    N, r, ew, n = shape
    c = case(*shape)
    seed = 20240607
    img = T(c["rn"])
    ft, oft = ingest.finish(img, r, c["std_n"], zero_mask=False, seed=seed, edge=ew)
    draws = philox_ref.mask_draws(seed, n, N)
    rl_check("finish-noise imgFT", shape, ft, opp.masked_image(c["rn"], r, c["std_n"], ew, draws))
    rl_check("finish-noise oriFT", shape, oft, c["ori"])
    img_b = T(c["rn"])
    ft_b, _ = ingest.finish(img_b, r, c["std_n"], zero_mask=False, seed=seed, edge=ew)
    assert torch.equal(torch.view_as_real(ft_b), torch.view_as_real(ft)) and torch.equal(img_b, img)
    img_z = T(c["rn"])
    _, oft_z = ingest.finish(img_z, r, c["std_n"], zero_mask=True, edge=ew)
    assert torch.equal(torch.view_as_real(oft_z), torch.view_as_real(oft))
    # finish masks in place: img now holds the masked, scaled real-space image
    img_c = T(c["rn"])
    ft_c, _ = ingest.finish(img_c, r, c["std_n"], zero_mask=False, seed=seed + 1, edge=ew)
    a, b, z, u = H(img), H(img_c), H(img_z), c["u"]
    rf = np.float32(r)
    assert np.all(a[:, u > rf] != b[:, u > rf])
    assert np.array_equal(a[:, u <= rf], b[:, u <= rf]) and np.array_equal(a[:, u <= rf], z[:, u <= rf])
    assert not torch.equal(torch.view_as_real(ft_c), torch.view_as_real(ft))


# ------------------------------------------------------------------- thx_remask
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_remask(shape):
    """reMaskImg on the masked transforms of the zero-mask step (nearly a fixed
    point: the mask applied twice) and on the transforms of arbitrary real
    images, where the mask removes most of the input."""
    N, r, ew, n = shape
    c = case(*shape)
    ft, _ = ingest.finish(T(c["rn"]), r, c["std_n"], zero_mask=True, keep_ori=False, edge=ew)
    before = H(ft).astype(np.complex128)
    ingest.remask(ft, r, edge=ew)
    rl_check("remask masked", shape, ft, opp.remask_image(before, N, r, ew))
    rng = np.random.default_rng(N)
    arb = np.fft.rfft2(rng.standard_normal((n, N, N)) + 0.5).astype(np.complex64)
    ft = T(arb)
    ingest.remask(ft, r, edge=ew)
    rl_check("remask arbitrary", shape, ft, opp.remask_image(arb.astype(np.complex128), N, r, ew))


def test_remask_wraps_the_grid():
    """One batch of 410 images at N = 36: 531 360 elements, more than the
    2048 x 256 threads of k_scale_mask_rl's launch."""
    shape = (36, 11.7, 6.0, 410)
    N, r, ew, n = shape
    assert n <= 512 and n * N * N > 2048 * 256
    rng = np.random.default_rng(36)
    arb = np.fft.rfft2(rng.standard_normal((n, N, N)) + 0.5).astype(np.complex64)
    ft = T(arb)
    ingest.remask(ft, r, edge=ew)
    rl_check("remask one batch", shape, ft, opp.remask_image(arb.astype(np.complex128), N, r, ew))


# --------------------------------------------------------------- thx_img_gather
def test_gather_wraps_the_grid():
    """allocPreCal's gather with every half-complex index of N = 32 in a
    shuffled order, 1000 images: 544 000 elements, more than the 2048 x 256
    threads of the launch; and the one- and zero-pixel sets."""
    N, n = 32, 1000
    rng = np.random.default_rng(5)
    ft = (rng.standard_normal((n, N, N // 2 + 1)) + 1j * rng.standard_normal((n, N, N // 2 + 1)))
    ft = ft.astype(np.complex64)
    ip = rng.permutation(N * (N // 2 + 1)).astype(np.int32)
    assert n * len(ip) > 2048 * 256
    d = T(ft)
    assert np.array_equal(H(ingest.gather(d, ip)), ft.reshape(n, -1)[:, ip])
    one = H(ingest.gather(d, ip[:1]))
    assert one.shape == (n, 1) and np.array_equal(one[:, 0], ft.reshape(n, -1)[:, ip[0]])
    assert ingest.gather(d, ip[:0]).shape == (n, 0)


# ---------------------------------------------------------------- thx_ctf_image
def ctf_attrs(n, seed):
    """CTF attribute rows {pixelSize, voltage, dU, dV, theta, Cs, ampC,
    phaseShift} that differ in every term, at a pixel size (3.3 A) that keeps
    the phase ki below 128 rad at the corner (N/2, -N/2) of the grid: K1
    defocus u^2 <= pi x 0.0251 x 3e4 x 2 / 6.6^2 = 109, K2 u^4 < 2.  The device
    and the C restatement form ki in float32, whose ulp there is 7.6e-6, so a
    few roundings that differ (fused multiply-adds, cosf) stay under the
    project's device-to-oracle CTF bound of 5e-5; at the 1.32 A of
    synth.ctf_attrs the corner's ki passes 512 rad, where one ulp is 6e-5."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), np.float32)
    a[:, 0] = 3.3
    a[:, 1] = np.where(np.arange(n) % 2, 200e3, 300e3)
    a[:, 2] = rng.uniform(15000, 30000, n)
    a[:, 3] = a[:, 2] - rng.uniform(500, 3000, n)
    a[:, 4] = rng.uniform(0, np.pi, n)
    a[:, 5] = np.where(np.arange(n) % 3, 2.7e7, 2.0e7)
    a[:, 6] = rng.uniform(0.07, 0.15, n)
    a[:, 7] = rng.uniform(0.0, 1.5, n)
    return a


def whole_grid(N):
    """Every stored pixel of the half-complex grid, made by hand: column iCol
    in [0, N/2], frequency row iRow in [-N/2, N/2) stored at row iRow mod N."""
    iRow, iCol = np.meshgrid(np.arange(-N // 2, N // 2), np.arange(N // 2 + 1), indexing="ij")
    iRow, iCol = iRow.reshape(-1).astype(np.int32), iCol.reshape(-1).astype(np.int32)
    iPxl = ((iRow % N) * (N // 2 + 1) + iCol).astype(np.int32)
    assert np.array_equal(np.sort(iPxl), np.arange(N * (N // 2 + 1)))
    return PixelSet(iCol, iRow, np.zeros_like(iCol), iPxl, 1)


def oracle_ctf_grid(orc, attr, N):
    px = whole_grid(N)
    ref = np.zeros((len(attr), N * (N // 2 + 1)), np.float32)
    for l, a in enumerate(attr):
        ref[l, px.iPxl] = orc.ctf(px, a, N)
    return ref.reshape(len(attr), N, N // 2 + 1)


def ctf_check(got, ref, N):
    assert got.shape == ref.shape
    print(f"MEASURED ctf N{N} worst {np.abs(got - ref).max():.3e}")
    assert np.max(np.abs(got - ref)) < 5e-5
    # the Nyquist column, and the row stored at N / 2 (frequency -N / 2)
    assert np.max(np.abs(got[:, :, N // 2] - ref[:, :, N // 2])) < 5e-5
    assert np.max(np.abs(got[:, N // 2, :] - ref[:, N // 2, :])) < 5e-5
    # the oracle's own rows tell -N / 2 from +N / 2 and row j from row N - j
    assert np.max(np.abs(ref[:, 1, 1:] - ref[:, N - 1, 1:])) > 0.1


@pytest.mark.parametrize("N", [16, 20])
def test_ctf_image_whole_grid(orc, N):
    attr = ctf_attrs(6, seed=N)
    ctf_check(H(ingest.ctf_images(T(attr), N)), oracle_ctf_grid(orc, attr, N), N)


def test_ctf_image_many_images(orc):
    """4000 images at N = 16 (4000 x 144 elements wraps the grid-stride loop)
    whose attribute rows cycle through 5: the first 5 against the oracle,
    every later image bit-equal to the one with its row."""
    N, n = 16, 4000
    base = ctf_attrs(5, seed=3)
    attr = base[np.arange(n) % 5]
    assert n * N * (N // 2 + 1) > 2048 * 256
    got = H(ingest.ctf_images(T(attr), N))
    ctf_check(got[:5], oracle_ctf_grid(orc, base, N), N)
    assert np.array_equal(got, got[:5][np.arange(n) % 5])


def test_gctfinit_whole_grid(orc):
    """thx_GCTFinit (host arrays, CTFAttr rows of 7 floats, one pixel size):
    (CTF, 0) over the whole grid against the oracle."""
    N, n = 16, 6
    attr = ctf_attrs(n, seed=4)
    ctfa = np.ascontiguousarray(attr[:, 1:])
    out = [np.full((N, N // 2 + 1), np.nan + 1j * np.nan, np.complex64) for _ in range(n)]
    arr = (ctypes.c_void_p * n)(*[x.ctypes.data for x in out])
    check(lib().thx_GCTFinit(arr, ctfa.ctypes.data_as(ctypes.c_void_p), float(attr[0, 0]), N, n),
          "GCTFinit")
    got = np.stack(out)
    assert np.all(got.imag == 0)
    ctf_check(np.ascontiguousarray(got.real), oracle_ctf_grid(orc, attr, N), N)
