"""numpy restatement of the image preprocessing (row f2), TEST INFRASTRUCTURE
ONLY (tests/), never imported by thunder_amd.  Parity status: "parity
unpinned" -- the reference ships no preprocessed fixtures; pinned here by
known answers (tests/test_ingest.py).

Follows, with the reference's compiled switches (OPTIMISER_MASK_IMG,
OPTIMISER_INIT_IMG_NORMALISE_OUT_MASK_REGION, include/Config.h:184, 190):
  ImageFile::readImage's centring (MESH_IMAGE_INDEX, include/Image/
    ImageFile.h:383-409): the stored image is rolled by -N/2 on both axes;
  substractBgImg (src/Optimiser.cpp:4928-4962) with bgMeanStddev
    (src/Image/ImageFunctions.cpp:607-620: pixels with i^2 + j^2 > r^2,
    GSL mean and sample sd);
  statImg's per-image terms (:4810-4905): bgStddev(0, img, r) (:585-596),
    stddev(0, img) (:543-547), regionMean(img, r, 0) (src/Functions/Mask.cpp:
    102-127);
  maskImg with zeroMask (:4964-4996) -> softMask(dst, src, r, ew, 0)
    (src/Functions/Mask.cpp:363-385), or without it the noise background
    softMask(dst, src, r, ew, 0, _stdN) (Mask.cpp:387-417) with the Gaussian
    draws passed in, normaliseImg (:4998-5012), fwImg (FFTW r2c,
    unnormalised);
  reMaskImg (:6093-6150): backward FFT / N^2, x softMask(mask, r, ew)
    (Mask.cpp:333-350), forward.
"""
import numpy as np

EDGE_WIDTH_RL = 6


def rl_coords(N):
    """(i, j) of every stored pixel in the corner-origin layout (Image::iRL)."""
    k = np.arange(N)
    c = np.where(k < N // 2, k, k - N)
    j, i = np.meshgrid(c, c, indexing="ij")
    return i, j


def load(img_centred):
    """The reference's read: centred on disk -> corner origin."""
    N = img_centred.shape[-1]
    return np.roll(img_centred, (-(N // 2), -(N // 2)), axis=(-2, -1))


def stats_and_normalise(img, r):
    """img: [N, N] corner origin, float32 -> (normalised float32 image,
    [bgMean, bgSd, bgStddev(0) after, stddev(0) after, mean inside r after])."""
    N = img.shape[-1]
    i, j = rl_coords(N)
    q = i.astype(np.float64) ** 2 + j.astype(np.float64) ** 2
    bg = q > r * r
    x = img.astype(np.float64)[bg]
    mean = x.mean()
    sd = np.sqrt(((x - mean) ** 2).sum() / (x.size - 1))
    fm, fsd = np.float32(mean), np.float32(sd)
    out = ((img.astype(np.float32) - fm) / fsd).astype(np.float32)
    o = out.astype(np.float64)
    b0 = np.sqrt((o[bg] ** 2).sum() / (bg.sum() - 1))
    a0 = np.sqrt((o ** 2).sum() / (o.size - 1))
    inside = np.sqrt(q) < r
    cm = o[inside].mean()
    return out, np.array([fm, fsd, b0, a0, cm], np.float64)


def soft_mask_keep(N, r, ew=EDGE_WIDTH_RL):
    i, j = rl_coords(N)
    u = np.hypot(i, j).astype(np.float32).astype(np.float64)
    w = 0.5 - 0.5 * np.cos((u - r) / ew * np.pi)          # portion of background
    return np.where(u < r, 1.0, np.where(u > r + ew, 0.0, 1.0 - w))


def masked_image(img, r, std_n, ew=EDGE_WIDTH_RL, draws=None):
    """maskImg + normaliseImg in real space, float64; img [..., N, N].
    draws None: zeroMask, softMask(dst, src, r, ew, 0).  Otherwise the
    noise background softMask(dst, src, r, ew, bgMean = 0, bgStd = stdN)
    (src/Functions/Mask.cpp:387-417): draws holds one standard normal per
    pixel (the caller's generator; the reference's is GSL's), the background
    draw * stdN replaces the image past r + ew and is blended in by the
    cosine weight over [r, r + ew]; inside r the draw is not used."""
    N = img.shape[-1]
    keep = soft_mask_keep(N, r, ew)
    x = img.astype(np.float64)
    if draws is None:
        return x * keep / std_n
    bg = np.asarray(draws, np.float64) * std_n
    return (bg * (1.0 - keep) + x * keep) / std_n


def finish(img, r, std_n, ew=EDGE_WIDTH_RL, draws=None):
    """softMask (zeroMask, or the noise background from draws) + 1 / stdN +
    forward FFT -> (imgFT, oriFT)."""
    o = img.astype(np.float64) / std_n
    return np.fft.rfft2(masked_image(img, r, std_n, ew, draws)), np.fft.rfft2(o)


def remask_image(ft, N, r, ew=EDGE_WIDTH_RL):
    """reMaskImg up to its forward transform: the re-masked real-space image."""
    rl = np.fft.irfft2(ft, s=(N, N))          # numpy's inverse is FFTW's backward / N^2
    return rl * soft_mask_keep(N, r, ew)


def remask(ft, N, r, ew=EDGE_WIDTH_RL):
    return np.fft.rfft2(remask_image(ft, N, r, ew))


# The real-space comparison of a half-complex result with a float64 image: a
# wrong mask weight at one pixel stays at that pixel here, where in Fourier
# space it is spread over every coefficient and measured against the DC term.
RL_TOL_MAX = 1e-5          # no tolerance of this comparison may exceed it


def rl_error(ft, ref_rl):
    """max |irfft2(ft) - ref| / max |ref| per image, in float64; ft
    [..., N, N/2+1] half-complex (unnormalised forward), ref_rl [..., N, N]."""
    ref = np.asarray(ref_rl, np.float64)
    rl = np.fft.irfft2(np.asarray(ft).astype(np.complex128), s=ref.shape[-2:])
    return np.abs(rl - ref).max(axis=(-2, -1)) / np.abs(ref).max(axis=(-2, -1))
