"""Post-processing on the device: THUNDER's ``thunder_postprocess``
(Postprocess::run, src/Postprocess.cpp:50-183) and its two small map tools,
``thunder_lowpass`` and ``thunder_bfactor``, over the kernels of
csrc/postprocess.hip and csrc/fsc_masked.hip.

    r = postprocess.postprocess(A_ft, B_ft, mask, pixel_size)    # device tensors in and out
    r.sharp, r.average, r.fsc, r.b_factor, r.resolution_A
    postprocess.run("a.mrc", "b.mrc", "mask.mrc", 1.32, "out/")  # the tool: MRC in, MRC out
    postprocess.low_pass(vol, pixel_size, 8.0)                   # thunder_lowpass
    postprocess.b_factor_filter(vol, -80.0)                      # thunder_bfactor

Maps are as everywhere in this package: half-complex complex64 [N, N, N/2+1]
unnormalised, real float32 [N, N, N] with the origin at [0, 0, 0]; N even,
16 <= N <= 1024.  The random phases of the FSC come from the package's Philox
stream keyed by ``seed``, so a call is reproducible bit for bit.
"""
import collections
import math
import os

import numpy as np
import torch

from . import io
from ._lib import check, lib
from .ops import _ptr, _req, _stream, workspace

B_FACTOR_EST_LOW_RES = 10.0     # Angstrom (include/Postprocess.h)
EDGE_WIDTH_FT = 4.0             # Fourier voxels

Postprocessed = collections.namedtuple(
    "Postprocessed", "fsc unmasked masked randomised thres res r_low n_fit status b_factor guinier "
    "average sharp resolution_A")


def _half_complex(A_ft, name="A_ft"):
    if A_ft.dim() != 3 or A_ft.shape[0] != A_ft.shape[1] or A_ft.shape[2] != A_ft.shape[0] // 2 + 1:
        raise ValueError(f"{name}: expected [N, N, N/2+1] half-complex, got {tuple(A_ft.shape)}")
    _req(A_ft, torch.complex64, None, name)
    return A_ft.shape[0]


def _cube(vol, name="vol"):
    if vol.dim() != 3 or len(set(vol.shape)) != 1:
        raise ValueError(f"{name}: expected [N, N, N], got {tuple(vol.shape)}")
    _req(vol, torch.float32, None, name)
    return vol.shape[0]


def postprocess(A_ft, B_ft, mask, pixel_size, seed=0, b_factor=None, low_res=B_FACTOR_EST_LOW_RES,
                edge_ft=EDGE_WIDTH_FT, method=0, want_average=True):
    """thx_postprocess: the FSC with phase randomisation, the 0.143 shell, the
    Guinier fit over [r_low, res) of the FSC-weighted merged map (skipped when
    ``b_factor`` is given), and the sharpened, low-passed, masked map.  Returns
    the named tuple (fsc, unmasked, masked, randomised: float64 [N/2-1] device
    tensors; thres, res, r_low, n_fit, status, b_factor: Python numbers from the
    one read-back after everything is enqueued; guinier: float64 [2, n_fit] of
    x = (u/N)^2 and y = log mean|F|; average (None without want_average), sharp:
    float32 [N, N, N]; resolution_A = N pixel_size / res)."""
    N = _half_complex(A_ft)
    _req(B_ft, torch.complex64, tuple(A_ft.shape), "B_ft")
    _req(mask, torch.float32, (N, N, N), "mask")
    dev = A_ft.device
    n_shell = N // 2 - 1
    f64 = dict(dtype=torch.float64, device=dev)
    fsc = torch.empty(n_shell, **f64)
    curves = torch.empty(3, n_shell, **f64)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    fit = torch.empty(4, **f64)
    guinier = torch.empty(2, n_shell, **f64)
    sharp = torch.empty(N, N, N, dtype=torch.float32, device=dev)
    average = torch.empty_like(sharp) if want_average else None
    with torch.cuda.device(dev):
        need = lib().thx_postprocess_workspace(N, n_shell, int(bool(want_average)))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)   # large: not kept in the cache
        check(lib().thx_postprocess(_ptr(A_ft), _ptr(B_ft), N, n_shell, _ptr(mask), float(pixel_size),
                                    float(low_res), float(edge_ft),
                                    float("nan") if b_factor is None else float(b_factor), int(seed),
                                    int(method), _ptr(fsc), _ptr(curves), _ptr(info), _ptr(fit),
                                    _ptr(guinier), _ptr(average), _ptr(sharp), _ptr(ws), need,
                                    _stream(dev)), "thx_postprocess")
    t, res, r_low, n_fit = (int(v) for v in info.cpu())
    b, _, _, status = (float(v) for v in fit.cpu())
    return Postprocessed(fsc, curves[0], curves[1], curves[2], t, res, r_low, n_fit, int(status), b,
                         guinier[:, :n_fit], average, sharp,
                         N * float(pixel_size) / res if res > 0 else math.inf)


def _fw(vol):
    """FFT::fw of a real map (thx_fft3d; torch's rfftn for a box it refuses)"""
    N = vol.shape[0]
    if N % 2:
        return torch.fft.rfftn(vol).to(torch.complex64).contiguous()
    C = torch.empty(N, N, N // 2 + 1, dtype=torch.complex64, device=vol.device)
    rl = vol.clone()
    with torch.cuda.device(vol.device):
        ws = workspace(lib().thx_fft3d_workspace(N), vol.device)
        check(lib().thx_fft3d(_ptr(C), _ptr(rl), N, 0, 0, _ptr(ws), ws.numel(), _stream(vol.device)),
              "thx_fft3d")
    return C


def _bw(C, N):
    """FFT::bw (C is overwritten), with its 1 / N^3"""
    rl = torch.empty(N, N, N, dtype=torch.float32, device=C.device)
    with torch.cuda.device(C.device):
        ws = workspace(lib().thx_fft3d_workspace(N), C.device)
        check(lib().thx_fft3d(_ptr(C), _ptr(rl), N, 1, 0, _ptr(ws), ws.numel(), _stream(C.device)),
              "thx_fft3d")
    return rl.mul_(1.0 / (float(N) ** 3))


def ft_sharpen(src_ft, b_factor=0.0, thres=-1.0, ew=0.0, out=None):
    """thx_ft_sharpen on a half-complex map: times exp(-0.5 b f^2), then the low
    pass (thres, ew in 1 / box; ew <= 0 or thres < 0: none).  b_factor / thres
    may be device tensors (float64 [1] / int32 [1], thres then a shell)."""
    N = _half_complex(src_ft, "src_ft")
    dst = torch.empty_like(src_ft) if out is None else out
    b_dev = b_factor if torch.is_tensor(b_factor) else None
    t_dev = thres if torch.is_tensor(thres) else None
    with torch.cuda.device(src_ft.device):
        check(lib().thx_ft_sharpen(_ptr(src_ft), N, 0.0 if b_dev is not None else float(b_factor),
                                   _ptr(b_dev), 0.0 if t_dev is not None else float(thres), _ptr(t_dev),
                                   float(ew), _ptr(dst), _stream(src_ft.device)), "thx_ft_sharpen")
    return dst


def low_pass(vol, pixel_size, freq_A):
    """thunder_lowpass (appsrc/thunder_lowpass.cpp:146-150): fw, lowPassFilter
    with thres = pixel_size / freq_A and ew = 2 / N, bw."""
    N = _cube(vol)
    thres = np.float32(pixel_size) / np.float32(freq_A)
    C = _fw(vol)
    return _bw(ft_sharpen(C, 0.0, float(thres), float(np.float32(2.0 / N)), out=C), N)


def b_factor_filter(vol, b):
    """thunder_bfactor: fw, bFactorFilter (times exp(-0.5 b f^2)), bw."""
    N = _cube(vol)
    C = _fw(vol)
    return _bw(ft_sharpen(C, float(b), out=C), N)


def check_sizes(shapes):
    """the constructor's check (Postprocess.cpp:33-47): three cubic maps of one size"""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    for s in shapes:
        if len(s) != 3 or len(set(s)) != 1:
            raise ValueError(f"postprocess: a map of shape {s} is not cubic")
    if len(set(shapes)) != 1:
        raise ValueError(f"postprocess: the maps differ in size: {shapes}")
    return shapes[0][0]


def write_fsc(path, fsc, N, pixel_size):
    """saveFSC (Postprocess.cpp:220-232): shell, 1 / Angstrom, FSC from shell 1"""
    f = np.asarray(fsc, np.float64)
    with open(path, "w") as fh:
        for i in range(1, len(f)):
            fh.write("%05d   %10.6f   %10.6f\n" % (i, i / (N * float(pixel_size)), f[i]))
    return path


def run(map_a, map_b, mask, pixel_size, out_dir, device="cuda:0", **kw):
    """thunder_postprocess: reads the two half-maps and the mask (MRC, centred
    layout), writes Reference_Average.mrc, Reference_Sharp.mrc and
    Postprocess_FSC.txt into out_dir and returns postprocess()'s tuple.  The
    reference's Reference_A_Masked.mrc / Reference_B_Masked.mrc are not written
    (as coded there they hold the unmasked inputs)."""
    maps = [io.read_mrc(p)[1] for p in (map_a, map_b, mask)]
    N = check_sizes([m.shape for m in maps])
    dev = torch.device(device)
    # centred -> origin at index 0: the inverse of mask.save_mask's fftshift
    a, b, m = (torch.as_tensor(np.fft.ifftshift(np.asarray(v, np.float32)).copy(), device=dev)
               for v in maps)
    r = postprocess(_fw(a), _fw(b), m, pixel_size, **kw)
    os.makedirs(out_dir, exist_ok=True)
    if r.average is not None:
        io.write_mrc(os.path.join(out_dir, "Reference_Average.mrc"),
                     np.fft.fftshift(r.average.cpu().numpy()), pixel_size)
    io.write_mrc(os.path.join(out_dir, "Reference_Sharp.mrc"), np.fft.fftshift(r.sharp.cpu().numpy()),
                 pixel_size)
    write_fsc(os.path.join(out_dir, "Postprocess_FSC.txt"), r.fsc.cpu().numpy(), N, pixel_size)
    return r
