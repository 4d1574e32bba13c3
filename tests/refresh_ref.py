"""numpy restatement of the round's last stage, written from the reference:

  average    Model::compareTwoHemispheres, src/Model.cpp:647-689
  low_pass   lowPassFilter, src/Functions/Filter.cpp:46-92
  soft_mask  softMask(dst, src, r, ew, bg = 0), src/Functions/Mask.cpp:499-521
  alpha_mask softMask(dst, src, alpha, bg = 0), :533-544
  pad_rl     VOL_PAD_RL / IMG_PAD_RL, include/Image/ImageFunctions.h:176-192
  grid_correction  Projector::gridCorrection, src/Projector.cpp:524-606
  projectee  solventFlatten's mask, then Projector::setProjectee
             (src/Projector.cpp:97-148): bw, pad, grid correction, fw

Everything is explicit in signed coordinates (index arrays of the wrapped
layouts).  ``dtype`` is the working precision: float64 is the reference,
float32 the same code in the device's precision, whose distance from float64
(e32) sets the scale of the GPU tests' bound.  Nothing here calls the library
or thunder_amd.synth.
"""
import numpy as np


def signed(n):
    """Signed coordinate of every wrapped index of a box n: [0, n/2), then [-n/2, 0)."""
    a = np.arange(n)
    return np.where(a < n // 2, a, a - n)


def _cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def _norm_rl(n, dims, dtype):
    """|(i, j[, k])| on the real-space grid of box n (NORM / NORM_3 of integers)."""
    s = signed(n).astype(np.float64)
    q = s[:, None] ** 2 + s[None, :] ** 2 if dims == 2 else (
        s[:, None, None] ** 2 + s[None, :, None] ** 2 + s[None, None, :] ** 2)
    return np.sqrt(q.astype(dtype))


def _quad_ft(n, dims):
    """i^2 + j^2 (+ k^2) on the half-complex grid [(k,) j, i <= n/2] (integers)."""
    s = signed(n)
    i = np.arange(n // 2 + 1)
    if dims == 2:
        return s[:, None] ** 2 + i[None, :] ** 2
    return s[:, None, None] ** 2 + s[None, :, None] ** 2 + i[None, None, :] ** 2


def average(A, B, r=None, dims=3, dtype=np.float64):
    """Both maps become (A + B) / 2 where QUAD < r^2 (r None or negative:
    everywhere); returns the new (A, B)."""
    c = _cdtype(dtype)
    A, B = np.asarray(A).astype(c), np.asarray(B).astype(c)
    avg = (A + B) / c(2)
    if r is None or r < 0:
        return avg.copy(), avg.copy()
    sel = _quad_ft(A.shape[-2], dims) < dtype(r) * dtype(r)
    return np.where(sel, avg, A), np.where(sel, avg, B)


def low_pass_weight(f, thres, ew, dtype=np.float64):
    f = np.asarray(f, dtype)
    thres, ew = dtype(thres), dtype(ew)
    edge = np.cos((f - thres) * dtype(np.pi) / ew) / dtype(2) + dtype(0.5)
    return np.where(f < thres, dtype(1), np.where(f > thres + ew, dtype(0), edge)).astype(dtype)


def low_pass(F, thres, ew, dims=3, dtype=np.float64):
    n = F.shape[-2]
    s = (signed(n).astype(dtype)) / dtype(n)
    i = (np.arange(n // 2 + 1).astype(dtype)) / dtype(n)
    q = s[:, None] ** 2 + i[None, :] ** 2 if dims == 2 else (
        s[:, None, None] ** 2 + s[None, :, None] ** 2 + i[None, None, :] ** 2)
    f = np.sqrt(q.astype(dtype))
    return (np.asarray(F).astype(_cdtype(dtype)) * low_pass_weight(f, thres, ew, dtype)).astype(_cdtype(dtype))


def soft_mask_weight(u, r, ew, dtype=np.float64):
    """1 - w of softMask with bg = 0: the share of the source that stays."""
    u = np.asarray(u, dtype)
    r, ew = dtype(r), dtype(ew)
    w = dtype(0.5) - dtype(0.5) * np.cos((u - r) / ew * dtype(np.pi))
    return np.where(u > r + ew, dtype(0), np.where(u >= r, dtype(1) - w, dtype(1))).astype(dtype)


def soft_mask(src, r, ew, dims=3, dtype=np.float64):
    src = np.asarray(src, dtype)
    return (src * soft_mask_weight(_norm_rl(src.shape[-1], dims, dtype), r, ew, dtype)).astype(dtype)


def alpha_mask(src, alpha, dtype=np.float64):
    w = dtype(1) - np.asarray(alpha, dtype)            # portion of background
    return (np.asarray(src, dtype) * (dtype(1) - w)).astype(dtype)


def pad_rl(src, pf):
    """Voxel (i, j, k), signed, to the same signed coordinate of the pf n box."""
    n = src.shape[-1]
    v = pf * n
    idx = signed(n) % v                                 # wrapped index in the padded box
    dims = src.ndim
    dst = np.zeros((v,) * dims, src.dtype)
    dst[np.ix_(*([idx] * dims))] = src
    return dst


def j0(x):
    x = np.asarray(x)
    safe = np.where(x == 0, 1, x)
    return np.where(x == 0, x.dtype.type(1), np.sin(safe) / safe)


def kernel_rl(u_over, interp="linear", dtype=np.float64):
    """TIK_RL (linear) or NIK_RL (nearest) of r = u_over."""
    s = j0(dtype(np.pi) * np.asarray(u_over, dtype)).astype(dtype)
    return s * s if interp == "linear" else s


def grid_correction(pad, pf, interp="linear", dtype=np.float64):
    """Divide by TIK_RL(|r| / (pf nColRL)), nColRL = the padded box."""
    v = pad.shape[-1]
    u = _norm_rl(v, pad.ndim, dtype)
    return (pad / kernel_rl(u / dtype(pf * v), interp, dtype)).astype(dtype)


def bw(F, dims=3, dtype=np.float64):
    """FFT::bw: the normalised inverse transform of a half-complex map."""
    n = F.shape[-2]
    return np.fft.irfftn(np.asarray(F).astype(_cdtype(dtype)), s=(n,) * dims,
                         axes=tuple(range(-dims, 0))).astype(dtype)


def projectee(ref, pf=2, mask_radius=None, mask=None, edge=6, interp="linear", scale=1.0,
              dtype=np.float64, dims=3):
    """One reference (real [n]*dims, or complex half-complex: bw first) ->
    the half-complex projectee of box pf n, times scale."""
    ref = np.asarray(ref)
    rl = bw(ref, dims, dtype) if np.iscomplexobj(ref) else ref.astype(dtype)
    if mask is not None:
        assert mask_radius is None and dims == 3
        rl = alpha_mask(rl, mask, dtype)
    elif mask_radius is not None:
        rl = soft_mask(rl, mask_radius, edge, dims, dtype)
    pad = grid_correction(pad_rl(rl, pf), pf, interp, dtype)
    return (np.fft.rfftn(pad) * dtype(scale)).astype(_cdtype(dtype))


def projectee2d(refs, pf=2, mask_radius=None, edge=6, interp="linear", scale=1.0, dtype=np.float64):
    return np.stack([projectee(r, pf, mask_radius, None, edge, interp, scale, dtype, dims=2)
                     for r in refs])


def single_voxel(n, pf, pos, w=1.0, mask_radius=None, edge=6, interp="linear"):
    """Closed form of projectee() for a map that is w at the signed voxel pos
    and 0 elsewhere: w m(|r|) / kernel(|r| / (pf vdim)) exp(-2 pi i k.r / vdim)
    at every stored frequency, in float64 scalar arithmetic."""
    import math
    dims = len(pos)                                      # pos = (i, j[, k]): column first
    v = pf * n
    u = math.sqrt(sum(p * p for p in pos))
    m = 1.0
    if mask_radius is not None:
        if u > mask_radius + edge:
            m = 0.0
        elif u >= mask_radius:
            m = 1.0 - (0.5 - 0.5 * math.cos((u - mask_radius) / edge * math.pi))
    x = math.pi * u / (pf * v)
    s = 1.0 if x == 0 else math.sin(x) / x
    amp = w * m / (s * s if interp == "linear" else s)
    ks = signed(v).astype(np.float64)
    ki = np.arange(v // 2 + 1, dtype=np.float64)
    if dims == 2:
        ph = ki[None, :] * pos[0] + ks[:, None] * pos[1]
    else:
        ph = ki[None, None, :] * pos[0] + ks[None, :, None] * pos[1] + ks[:, None, None] * pos[2]
    return amp * np.exp(-2j * np.pi * ph / v)
