"""The last stage of a round on the device: the reconstructed reference of
box N becomes the next round's projectee of box pf N (csrc/refresh.hip).

average_halves   Model::compareTwoHemispheres' averaging (src/Model.cpp:611-690)
                 and, optionally, lowPassFilter (src/Functions/Filter.cpp:46-92)
refresh_projectee  Optimiser::solventFlatten's mask (src/Optimiser.cpp:7768-7989)
                 + Model::refreshProj -> Projector::setProjectee
                 (src/Model.cpp:1013-1044, src/Projector.cpp:97-148): pad,
                 grid correction, unnormalised forward transform

The result has the layout ops._vol_dim / ops._img2d_dim check and feeds
Expectation, ops.project3d and ops.local_phase2d as it is.
"""
import math

import torch

from ._lib import check, lib
from .ops import _ptr, _req, _stream, workspace

_METHODS = {"auto": 0, "fallback": 1, "pruned": 2}
_INTERP = {"linear": 0, "nearest": 1}


def average_halves(A_ft, B_ft=None, r=None, low_pass=None, mode2d=False):
    """In place on the Fourier maps of the two hemispheres: A = B = (A + B) / 2
    where i^2 + j^2 + k^2 < r^2 (r None: everywhere, the K > 1 / no-gold-standard
    branch), then the low-pass ``low_pass = (thres, ew)`` in units of 1 / N
    (None: off, as the reference compiles it).  B_ft None skips the averaging.
    Maps: complex64 [N, N, N/2+1] or [nK, N, N, N/2+1]; mode2d: images
    [N, N/2+1] or [nK, N, N/2+1]."""
    base = 2 if mode2d else 3
    if A_ft.dim() not in (base, base + 1):
        raise ValueError(f"A_ft: expected {base} axes (+ a leading class axis), got {tuple(A_ft.shape)}")
    N = A_ft.shape[-2]
    want = (N,) * (base - 1) + (N // 2 + 1,)
    if tuple(A_ft.shape[-base:]) != want:
        raise ValueError(f"A_ft: expected [..., {', '.join(map(str, want))}], got {tuple(A_ft.shape)}")
    _req(A_ft, torch.complex64, None, "A_ft")
    if B_ft is not None:
        _req(B_ft, torch.complex64, tuple(A_ft.shape), "B_ft")
        if B_ft.device != A_ft.device:
            raise ValueError("B_ft: on another device")
    nK = A_ft.shape[0] if A_ft.dim() == base + 1 else 1
    thres, ew = (0.0, 1.0) if low_pass is None else map(float, low_pass)
    with torch.cuda.device(A_ft.device):
        check(lib().thx_ref_average(_ptr(A_ft), _ptr(B_ft), N, nK, -1.0 if r is None else float(r),
                                    thres, ew, 0 if mode2d else 1, _stream(A_ft.device)),
              "thx_ref_average")
    return A_ft, B_ft


def refresh_projectee(ref, pf=2, mask_radius=None, mask=None, edge=6, interp="linear", scale=1.0,
                      method="auto", out=None, mode2d=False):
    """The projectee of the reference ``ref``.

    3D: ref float32 [N, N, N] (real space, origin at [0, 0, 0], negatives
    wrapped: ops.reconstruct's map) or complex64 [N, N, N/2+1] (its transform)
    -> complex64 [pf N, pf N, pf N/2+1]; a leading class axis loops.
    mode2d: ref float32 [nK, N, N] or complex64 [nK, N, N/2+1] -> [nK, pf N,
    pf N/2+1].  mask_radius / edge: the radial soft mask (pixels); mask: a
    provided [N, N, N] alpha volume in [0, 1] (3D only); neither: no mask.
    scale multiplies the result (1: the reference's unnormalised transform,
    N ** -1.5: the synthetic projectees' normalisation).  method: "auto",
    "fallback" (fused pad + hipFFT) or "pruned" (the LDS passes that skip the
    zero lines; power-of-two pf N <= 512).  Stream-ordered."""
    if method not in _METHODS:
        raise ValueError(f"method: one of {sorted(_METHODS)}")
    if interp not in _INTERP:
        raise ValueError(f"interp: one of {sorted(_INTERP)}")
    if not isinstance(ref, torch.Tensor) or not ref.is_cuda:
        raise ValueError("ref: must be a device tensor")
    if ref.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"ref: dtype {ref.dtype}, expected float32 or complex64")
    from_ft = ref.dtype == torch.complex64
    _req(ref, ref.dtype, None, "ref")
    if mask is not None and mask_radius is not None:
        raise ValueError("mask_radius and mask are exclusive")
    r_mask = 0.0 if mask_radius is None else float(mask_radius)
    if mask_radius is not None and not (r_mask > 0 and math.isfinite(r_mask)):
        raise ValueError("mask_radius: must be positive")
    dev = ref.device
    L = lib()
    if mode2d:
        if ref.dim() == 2:
            ref = ref.unsqueeze(0)
        if ref.dim() != 3:
            raise ValueError(f"ref (2D): expected [nK, N, N] or [nK, N, N/2+1], got {tuple(ref.shape)}")
        if mask is not None:
            raise ValueError("a provided mask is 3D only")
        nK, N = ref.shape[0], ref.shape[1]
        if ref.shape[2] != (N // 2 + 1 if from_ft else N):
            raise ValueError(f"ref (2D): bad shape {tuple(ref.shape)}")
        vdim = pf * N
        shape = (nK, vdim, vdim // 2 + 1)
        out = torch.empty(shape, dtype=torch.complex64, device=dev) if out is None else _req(
            out, torch.complex64, shape, "out")
        with torch.cuda.device(dev):
            ws = workspace(L.thx_projectee2d_workspace(N, pf, nK, int(from_ft)), dev)
            check(L.thx_projectee2d(_ptr(ref), int(from_ft), nK, N, pf, r_mask, float(edge), None,
                                    _INTERP[interp], float(scale), _ptr(out), _ptr(ws), ws.numel(),
                                    _stream(dev)), "thx_projectee2d")
        return out
    if ref.dim() == 4:
        N = ref.shape[1]
        vdim = pf * N
        shape = (ref.shape[0], vdim, vdim, vdim // 2 + 1)
        out = torch.empty(shape, dtype=torch.complex64, device=dev) if out is None else _req(
            out, torch.complex64, shape, "out")
        for c in range(ref.shape[0]):
            refresh_projectee(ref[c], pf, mask_radius, mask, edge, interp, scale, method, out[c])
        return out
    if ref.dim() != 3 or ref.shape[0] != ref.shape[1] or ref.shape[2] != (
            ref.shape[0] // 2 + 1 if from_ft else ref.shape[0]):
        raise ValueError(f"ref: expected [N, N, N] real or [N, N, N/2+1] complex, got {tuple(ref.shape)}")
    N = ref.shape[0]
    vdim = pf * N
    if mask is not None:
        _req(mask, torch.float32, (N, N, N), "mask")
        if mask.device != dev:
            raise ValueError("mask: on another device")
    shape = (vdim, vdim, vdim // 2 + 1)
    out = torch.empty(shape, dtype=torch.complex64, device=dev) if out is None else _req(
        out, torch.complex64, shape, "out")
    need = L.thx_projectee_workspace(N, pf, _METHODS[method], int(from_ft))
    if need == 0:
        raise ValueError(f"refresh_projectee: N = {N}, pf = {pf}, method = {method!r} is not supported")
    with torch.cuda.device(dev):
        ws = workspace(need, dev)
        check(L.thx_projectee(_ptr(ref), int(from_ft), N, pf, r_mask, float(edge), _ptr(mask),
                              _INTERP[interp], float(scale), _ptr(out), _METHODS[method], _ptr(ws),
                              ws.numel(), _stream(dev)), "thx_projectee")
    return out
