"""f2 ingest on the CPU: the MRC2014 and .thu I/O of thunder_amd.io, and the
numpy restatement of the image preprocessing (oracle/preprocess.py) pinned by
known answers (the reference holds no preprocessed fixtures: parity
unpinned).  The device path is tests/test_gpu_ingest.py."""
import struct

import numpy as np
import pytest

import philox_ref
from oracle import preprocess as opp
from thunder_amd import io


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.float16, np.uint16, np.int8])
def test_mrc_round_trip(tmp_path, dtype):
    rng = np.random.default_rng(1)
    a = (rng.standard_normal((5, 24, 32)) * 40).astype(dtype)
    p = tmp_path / "s.mrcs"
    io.write_mrc(p, a, pixel_size=1.32)
    h, d = io.read_mrc(p)
    assert (h.nx, h.ny, h.nz) == (32, 24, 5)
    assert h.mode == {np.float32: 2, np.int16: 1, np.float16: 12, np.uint16: 6, np.int8: 0}[dtype]
    assert abs(h.pixel_size - 1.32) < 1e-6
    assert np.array_equal(np.asarray(d), a)
    raw = p.read_bytes()
    assert len(raw) == 1024 + a.nbytes and raw[208:212] == b"MAP "


def test_mrc_big_endian_and_extended_header(tmp_path):
    """A big-endian file (machine stamp 0x11 0x11) with an extended header of
    NSYMBT bytes: the data start after it and are byte-swapped on read."""
    rng = np.random.default_rng(2)
    a = rng.standard_normal((3, 8, 8)).astype(np.float32)
    h = io.MrcHeader(8, 8, 3, 2, cella=(8.0, 8.0, 3.0), nsymbt=96, byteorder=">")
    p = tmp_path / "be.mrc"
    p.write_bytes(h.pack() + bytes(96) + a.astype(">f4").tobytes())
    h2, d = io.read_mrc(p, mmap=False)
    assert h2.byteorder == ">" and h2.nsymbt == 96 and h2.mode == 2
    assert np.array_equal(d.astype(np.float32), a)
    # NX / MODE are the first words, per the spec
    assert struct.unpack(">4i", p.read_bytes()[:16]) == (8, 8, 3, 2)


def test_thu_round_trip_and_ctf_attrs(tmp_path):
    rng = np.random.default_rng(3)
    n = 7
    ctf = np.stack([np.full(n, 300e3), rng.uniform(1e4, 3e4, n), rng.uniform(1e4, 3e4, n),
                    rng.uniform(0, np.pi, n), np.full(n, 2.7e7), np.full(n, 0.1), np.zeros(n)], 1)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = io.thu_table(n, [f"{i + 1:06d}@stack.mrcs" for i in range(n)], ctf, q,
                     rng.standard_normal((n, 2)), group=np.arange(n) % 3)
    p = tmp_path / "p.thu"
    io.write_thu(p, t)
    lines = p.read_text().splitlines()
    assert len(lines) == n and all(len(ln.split()) == 27 for ln in lines)
    r = io.read_thu(p)
    assert r["particlePath"] == t["particlePath"]
    for name in io.THU_COLUMNS:
        if name not in ("particlePath", "micrographPath"):
            assert np.allclose(r[name], t[name], rtol=0, atol=5e-9 * max(1.0, np.abs(t[name]).max()))
    a = io.thu_ctf_attrs(r, 1.32)
    assert a.shape == (n, 8) and np.allclose(a[:, 0], 1.32) and np.allclose(a[:, 2], ctf[:, 1])


def test_thu_rejects_short_rows(tmp_path):
    p = tmp_path / "bad.thu"
    p.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        io.read_thu(p)


def test_load_images_from_stacks(tmp_path):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((4, 16, 16)).astype(np.float32)
    b = rng.standard_normal((1, 16, 16)).astype(np.float32)
    io.write_mrc(tmp_path / "a.mrcs", a)
    io.write_mrc(tmp_path / "b.mrc", b)
    t = io.thu_table(3, ["000003@a.mrcs", "b.mrc", "1@a.mrcs"])
    imgs = io.load_images(t, str(tmp_path))
    assert np.array_equal(imgs[0], a[2]) and np.array_equal(imgs[1], b[0])
    assert np.array_equal(imgs[2], a[0])


def test_preprocess_restatement_known_answers():
    """Background N(7, 3^2) outside the mask radius, a bright disc inside:
    after substractBgImg the background has mean 0 and sample sd 1 (so
    statImg's bgStddev(0) is 1), the stored image is the centred one rolled
    by N/2, the soft mask is 1 inside r, 0 past r + 6 and 1/2 half-way, and
    the forward transform is numpy's unnormalised rfft2."""
    N, r = 64, 20.0
    rng = np.random.default_rng(5)
    c = (rng.standard_normal((N, N)) * 3 + 7).astype(np.float32)
    yy, xx = np.mgrid[:N, :N] - N // 2
    c[np.hypot(xx, yy) < 10] += 50
    img = opp.load(c)
    assert img[0, 0] == c[N // 2, N // 2]
    out, st = opp.stats_and_normalise(img, r)
    i, j = opp.rl_coords(N)
    bg = i.astype(float) ** 2 + j.astype(float) ** 2 > r * r
    assert abs(out[bg].astype(np.float64).mean()) < 1e-6
    assert abs(st[2] - 1.0) < 1e-6 and abs(st[0] - 7) < 0.2 and abs(st[1] - 3) < 0.1
    keep = opp.soft_mask_keep(N, r)
    u = np.hypot(i, j)
    assert np.all(keep[u < r] == 1) and np.all(keep[u > r + 6] == 0)
    half = np.isclose(u, r + 3)
    assert half.any() and np.allclose(keep[half], 0.5, atol=1e-6)
    ft, oft = opp.finish(out, r, 1.0)
    assert np.allclose(oft, np.fft.rfft2(out.astype(np.float64)))
    # re-masking an image supported inside r changes nothing
    inner = np.where(u < r, out, 0).astype(np.float64)
    assert np.allclose(opp.remask(np.fft.rfft2(inner), N, r), np.fft.rfft2(inner), atol=1e-9)


def _normalised_image(N, r, seed):
    """A smooth blob plus noise with an offset and a gain, through substractBgImg."""
    rng = np.random.default_rng(seed)
    i, j = opp.rl_coords(N)
    blob = np.exp(-(i ** 2 + j ** 2) / (2 * (N / 6.0) ** 2))
    img = (1.7 * (3 * blob + 0.5 * rng.standard_normal((N, N))) + 2.0).astype(np.float32)
    out, st = opp.stats_and_normalise(img, r)
    return out, float(st[2])


def test_noise_mask_restatement_known_answers():
    """softMask(dst, src, r, ew, bgMean = 0, bgStd = stdN) then 1 / stdN, at
    N = 32, r = 7, ew = 6, where lattice points lie on r, on r + ew / 2 = 10
    and on r + ew = 13: inside r the pixel is untouched, on r the background's
    weight is 0, half-way it is the half-and-half blend, on and beyond r + ew
    it is draw * stdN / stdN; with all draws zero it is the zero mask; finish
    is the rfft2 of the masked image in both modes."""
    N, r, ew = 32, 7.0, 6.0
    x, std_n = _normalised_image(N, r, 11)
    g = np.random.default_rng(12).standard_normal((N, N))
    m = opp.masked_image(x, r, std_n, ew, draws=g)
    i, j = opp.rl_coords(N)
    u = np.hypot(i, j)
    xs = x.astype(np.float64) / std_n
    assert (u < r).sum() > 100 and np.array_equal(m[u < r], xs[u < r])
    assert (u == r).sum() == 4 and np.allclose(m[u == r], xs[u == r], rtol=0, atol=1e-15)
    assert (u > r + ew).sum() > 100
    assert np.allclose(m[u > r + ew], (g * std_n / std_n)[u > r + ew], rtol=1e-15, atol=0)
    assert (u == r + ew).sum() == 12 and np.allclose(m[u == r + ew], g[u == r + ew], rtol=1e-12)
    half = u == r + ew / 2
    assert half.sum() == 12 and np.allclose(m[half], 0.5 * g[half] + 0.5 * xs[half], rtol=0, atol=1e-12)
    edge = (u > r) & (u < r + ew)
    w = (m[edge] - xs[edge]) / (g[edge] - xs[edge])          # the background's portion
    assert np.all((w > 0) & (w < 1))
    zero = opp.masked_image(x, r, std_n, ew)
    assert np.array_equal(opp.masked_image(x, r, std_n, ew, draws=np.zeros((N, N))), zero)
    assert np.allclose(zero, xs * opp.soft_mask_keep(N, r, ew), rtol=1e-15, atol=0)
    for d in (None, g):
        ft, oft = opp.finish(x, r, std_n, ew, draws=d)
        assert np.array_equal(ft, np.fft.rfft2(opp.masked_image(x, r, std_n, ew, draws=d)))
        assert np.array_equal(oft, np.fft.rfft2(xs))
    # re-masking: remask is the rfft2 of remask_image
    assert np.array_equal(opp.remask(ft, N, r, ew), np.fft.rfft2(opp.remask_image(ft, N, r, ew)))


def test_philox_restatement_known_answers():
    """Philox-4x32-10 at Random123's published vectors, uniform's 53-bit
    construction, and the mask stream's Box-Muller normals: mean and sd over
    the 513 x 32 x 32 draws of seed 1 within 5 standard errors of 0 and 1."""
    x = philox_ref._philox_4x32_10(0, 0, 0, 0, 0)
    assert [int(v) for v in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    x = philox_ref._philox_4x32_10((f << 32) | f, f, f, f, f)
    assert [int(v) for v in x] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # counter 0, key 0: x = 0x6627e8d5, y = 0xe169c58d
    m = ((0x6627E8D5 << 21) ^ 0xE169C58D) & ((1 << 53) - 1)
    assert philox_ref.uniform(0, 0, 0, 0, 0) == (m + 0.5) / 2.0 ** 53
    u1, u2 = philox_ref.uniform(5, 1, 2, 3, 0), philox_ref.uniform(5, 1, 2, 3, 1)
    assert philox_ref.gauss(5, 1, 2, 3) == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    g = philox_ref.mask_draws(1, 513, 32)
    n = g.size
    assert g.shape == (513, 32, 32) and np.all(np.isfinite(g))
    assert abs(g.mean()) < 5 / np.sqrt(n) and abs(g.std() - 1) < 5 / np.sqrt(2 * n)
    # pixel q's stream does not depend on the stack's size; another seed is another stream
    assert np.array_equal(philox_ref.mask_draws(1, 2, 32), g[:2])
    assert not np.any(philox_ref.mask_draws(2, 2, 32) == g[:2])


def test_real_space_comparison_sees_one_wrong_mask_weight():
    """Why tests/test_gpu_preprocess.py compares in real space: one edge
    pixel's mask weight off by 1e-3 (N = 36, r = 11.7, ew = 6) moves the
    Fourier output by less than the 2e-5 x max bound of
    test_gpu_ingest.py::test_preprocess_matches_restatement, because every
    coefficient is measured against the DC term; brought back with irfft2 the
    error stays at its pixel and fails the real-space bound, while a correct
    float32 output passes it."""
    N, r, ew = 36, 11.7, 6.0
    x, std_n = _normalised_image(N, r, 7)
    ref = opp.masked_image(x, r, std_n, ew)
    keep = opp.soft_mask_keep(N, r, ew)
    edge = (keep > 0.2) & (keep < 0.8)
    p = np.unravel_index(np.argmax(np.where(edge, np.abs(x), 0)), x.shape)
    wrong = keep.copy()
    wrong[p] += 1e-3
    ft_ref = np.fft.rfft2(ref)
    ft_bad = np.fft.rfft2(x.astype(np.float64) * wrong / std_n).astype(np.complex64)
    assert np.abs(ft_bad - ft_ref).max() <= 2e-5 * np.abs(ft_ref).max()          # unseen
    assert opp.rl_error(ft_bad, ref) > 10 * opp.RL_TOL_MAX                       # seen
    assert opp.rl_error(ft_ref.astype(np.complex64), ref) < 0.1 * opp.RL_TOL_MAX
