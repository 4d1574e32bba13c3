"""The reconstruction solve (oracle/reconstruct.py's reconstruct) restated in
torch, parametrised by dtype and device: float64 is the reference of the GPU
tests (on the device where the padded box is large), float32 -- every array
and every operation in float32, complex64 FFTs -- measures what float32
rounding alone does to the same solve, which is what the tests' bars are
made of.  tests/test_recon_ref.py pins the float64 form to the oracle.

Besides the map it returns what the balancing loop itself computes: the
weights W, T as the solve leaves it (MAP factor applied, floored at 1e-25),
the iteration count and max | |C| - 1 | after each iteration."""
import math

import numpy as np
import torch

from oracle import reconstruct as orc_rc


def _freq(n, dev):
    return torch.fft.fftfreq(n, 1.0 / n, device=dev, dtype=torch.float64).round().long()


def ft_quad(vdim, dev="cpu"):
    """|k|^2 on the half-complex grid [k][j][i] (int64)."""
    j = _freq(vdim, dev)
    i = torch.arange(vdim // 2 + 1, device=dev)
    return j[:, None, None] ** 2 + j[None, :, None] ** 2 + i[None, None, :] ** 2


def _rl_quad(n, dev):
    c = _freq(n, dev)
    return c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2


def max_r(N, a=1.9, max_radius=0):
    return max_radius if max_radius > 0 else N // 2 - int(math.ceil(a))


def map_factor(vdim, pf, maxR, fsc, join_half=False, dtype=torch.float64, device="cpu"):
    """The MAP Wiener factor T is divided by, per voxel of the half-complex
    grid: on shells 5 pf <= |k| < maxR pf the FSC at shell round(|k|) // pf
    (0 past its end) clamped to [1e-3, 1 - 1e-3], sqrt(2 f / (1 + f)) when
    joining halves; 1 elsewhere."""
    quad = ft_quad(vdim, device)
    m = (quad >= (5 * pf) ** 2) & (quad < (maxR * pf) ** 2)
    u = torch.round(torch.sqrt(quad[m].to(dtype))).long()
    idx = torch.div(u, pf, rounding_mode="floor")
    fs = torch.as_tensor(np.asarray(fsc, np.float64), device=device).to(dtype)
    f = torch.where(idx >= len(fs), torch.zeros((), dtype=dtype, device=device),
                    fs[torch.clamp(idx, max=len(fs) - 1)])
    f = torch.clamp(f, 1e-3, 1 - 1e-3)
    if join_half:
        f = torch.sqrt(2 * f / (1 + f))
    out = torch.ones(quad.shape, dtype=dtype, device=device)
    out[m] = f
    return out


def reconstruct(F, T, N, pf=2, a=1.9, alpha=15.0, grid_corr=True, max_radius=0, fsc=None,
                join_half=False, dtype=torch.float64, device=None):
    """F [vdim, vdim, vdim/2+1] complex, T the same shape real (numpy or torch).
    Returns (map [N, N, N], W, T_after: tensors of dtype on device;
    iterations; diffs)."""
    vdim = pf * N
    dev = torch.device(device) if device is not None else (
        F.device if torch.is_tensor(F) else torch.device("cpu"))
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    F = torch.as_tensor(F).to(device=dev, dtype=cdt)
    T = torch.as_tensor(T).to(device=dev, dtype=dtype).clone()
    maxR = max_r(N, a, max_radius)
    inside = ft_quad(vdim, dev) < (maxR * pf) ** 2
    if fsc is not None:
        T = T / map_factor(vdim, pf, maxR, fsc, join_half, dtype, dev)
    W = inside.to(dtype)
    T = torch.clamp(T, min=1e-25)
    diffs = []
    m = 0
    if grid_corr:
        tab = torch.as_tensor(orc_rc.mkb_rl_r2(np.arange(orc_rc.TAB_N + 1) * 1e-5, a, alpha)
                              .astype(np.float32), device=dev).to(dtype)
        nf = float(orc_rc.mkb_rl_r2(np.array([0.0]), a, alpha)[0])
        x = _rl_quad(vdim, dev).to(dtype) / float(vdim * vdim)
        kern = tab[torch.clamp(torch.round(x / 1e-5).long(), max=orc_rc.TAB_N)] / nf
        del x
        diff_prev = diff = float(np.finfo(np.float32).max)
        n_no = 0
        for m in range(30):
            C = (T * W).to(cdt)
            c = torch.fft.irfftn(C, s=(vdim, vdim, vdim)) * kern
            del C
            a_ = torch.fft.rfftn(c).abs()
            del c
            W = torch.where(inside, W / torch.clamp(a_, min=1e-6), W)
            diff_prev, diff = diff, float((a_[inside] - 1).abs().max())
            del a_
            diffs.append(diff)
            n_no = n_no + 1 if diff > diff_prev * 0.95 else 0
            if diff < 1e-2 or (m >= 10 and n_no == 2):
                m += 1
                break
        else:
            m = 30
        del kern
    else:
        W = torch.where(inside, 1.0 / torch.clamp(T.abs(), min=1e-6), W)
    pad = torch.where(inside, F * W, torch.zeros((), dtype=cdt, device=dev))
    rl = torch.fft.irfftn(pad, s=(vdim, vdim, vdim))
    del pad
    cN = _freq(N, dev) % vdim
    box = rl[cN][:, cN][:, :, cN]
    del rl
    x = math.pi * torch.sqrt(_rl_quad(N, dev).to(dtype)) / vdim
    one = torch.ones_like(x)
    j0 = torch.where(x == 0, one, torch.sin(x) / torch.where(x == 0, one, x))
    return box / (j0 * j0), W, T, m, diffs


def sampling_density(family, vdim, seed, p=0.0, flat=False):
    """T [vdim, vdim, vdim/2+1] float64 (numpy) of one of the test families,
    deliberately not Hermitian-symmetric on the kx = 0 and kx = vdim/2 planes:
      smooth:  50 / (1 + |k|) x U(0.8, 1.2);
      decades: the smooth base (or 1, flat) x 10^U(-p, p) per voxel;
      holes:   smooth with a random 10 % of voxels set to 0."""
    rng = np.random.default_rng(seed)
    quad = ft_quad(vdim).numpy().astype(np.float64)
    base = np.ones_like(quad) if flat else 50.0 / (1.0 + np.sqrt(quad))
    if family == "smooth":
        return base * rng.uniform(0.8, 1.2, quad.shape)
    if family == "decades":
        return base * 10.0 ** rng.uniform(-p, p, quad.shape)
    if family == "holes":
        T = base * rng.uniform(0.8, 1.2, quad.shape)
        T[rng.random(quad.shape) < 0.1] = 0.0
        return T
    raise ValueError(family)


def white_data(T, seed, device="cpu"):
    """F = T x rfftn(white real noise), made Hermitian-consistent by
    rfftn(irfftn(.)) in float64 (complex128 tensor on device): every shell
    carries equal weight in the map, and F's kx = 0 plane is a real volume's.
    The noise is numpy's, so the data are the same on every device; its sum
    (the one voxel of shell 0) is set to a coefficient's typical sqrt(vdim^3),
    so that no seed makes shell 0 of the map a difference of large numbers."""
    vdim = T.shape[0]
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((vdim, vdim, vdim))
    noise += (np.sqrt(noise.size) - noise.sum()) / noise.size
    noise = torch.as_tensor(noise, device=device)
    F = torch.as_tensor(T, device=device) * torch.fft.rfftn(noise)
    del noise
    return torch.fft.rfftn(torch.fft.irfftn(F, s=(vdim, vdim, vdim)))


def stop_margins(diffs):
    """How far the float64 diffs keep from the stopping rule's two thresholds:
    (min | diff[m] / diff[m-1] - 0.95 |, min | diff[m] - 1e-2 | / 1e-2).  A
    run whose margins are small may stop elsewhere in float32 for no fault."""
    d = np.asarray(diffs, np.float64)
    ratio = np.min(np.abs(d[1:] / d[:-1] - 0.95)) if len(d) > 1 else np.inf
    thres = np.min(np.abs(d - 1e-2)) / 1e-2 if len(d) else np.inf
    return float(ratio), float(thres)


def solve_errors(got, ref, inside):
    """Errors of a solve (map, W, diffs) against the float64 one, each in the
    metric the tests assert: the map over its maximum; W relative, the
    maximum over the sphere; a diff over max(1, diff) -- it is the deviation
    of |C| from 1, so its rounding error scales with max(1, |C|)."""
    (m, W, d), (rm, rW, rd) = got, ref
    rm, rW = rm.double(), rW.double()
    out = {"map": float((m.double() - rm).abs().max() / rm.abs().max()),
           "W": float(((W.double() - rW).abs()[inside] / rW[inside]).max())}
    if len(rd):
        d, rd = np.asarray(d, np.float64), np.asarray(rd, np.float64)
        out["diffs"] = float(np.max(np.abs(d - rd) / np.maximum(1.0, rd))) if len(d) == len(rd) else np.inf
    return out


def shell_errors(ft, ref_ft, N, maxR):
    """Relative L2 error of a map's transform [N, N, N/2+1] on each shell
    u = round(|k|) of 0 ... maxR - 1."""
    u = torch.round(torch.sqrt(ft_quad(N, ref_ft.device).double())).long()
    sel = u < maxR
    ref_ft = ref_ft.to(torch.complex128)
    num = torch.zeros(maxR, dtype=torch.float64, device=ref_ft.device)
    den = torch.zeros_like(num)
    num.index_add_(0, u[sel], ((ft.to(torch.complex128) - ref_ft).abs() ** 2)[sel])
    den.index_add_(0, u[sel], (ref_ft.abs() ** 2)[sel])
    return torch.sqrt(num / den).cpu().numpy()


def hermitian_plane_average(T):
    """T with its kx = 0 and kx = vdim/2 planes replaced by (T(k) + T(-k)) / 2,
    as the even half-grid balancing loop leaves them."""
    T = T.clone()
    for x in (0, T.shape[2] - 1):
        p = T[:, :, x]
        T[:, :, x] = 0.5 * (p + torch.roll(torch.flip(p, (0, 1)), (1, 1), (0, 1)))
    return T
