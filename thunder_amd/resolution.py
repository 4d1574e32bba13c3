"""The resolution estimate of a 3D refinement with ``maskFSC`` / ``coreFSC``:
the masked branch of Model::compareTwoHemispheres (src/Model.cpp:411-567) over
the kernels of csrc/fsc_masked.hip.

    r = resolution.masked_fsc(A_ft, B_ft, n_shell, mask=m)            # _maskFSC
    r = resolution.masked_fsc(A_ft, B_ft, n_shell, core_radius=40.0)  # _coreFSC
    r.fsc                                   # what the reference stores in _FSC
    resolution.res_p(r.fsc.cpu().numpy(), 0.143, inverse=True)

A_ft, B_ft: the two hemispheres' half-complex maps, complex64 [N, N, N/2+1];
they are read only.  The random phases come from the package's Philox stream
keyed by ``seed`` (the reference draws from an urandom-seeded generator), so a
call is reproducible bit for bit.
"""
import collections

import numpy as np
import torch

from ._lib import check, lib
from .ops import _ptr, _req, _stream

MaskedFSC = collections.namedtuple("MaskedFSC", "fsc unmasked masked randomised thres")


def res_p(fsc, thres, pf=1, rL=1, inverse=False):
    """resP (src/Functions/Spectrum.cpp:339-363) on the host: the last shell
    from rL whose FSC is not below thres (inverse: the last one above it,
    searched from the top), over pf; thres compares as the reference's RFLOAT."""
    f = np.asarray(fsc, np.float64)
    thr = float(np.float32(thres))
    if inverse:
        r = len(f) - 1
        while r >= rL and not f[r] > thr:
            r -= 1
    else:
        r = rL
        while r < len(f) and not f[r] < thr:
            r += 1
        r -= 1
    return int(r / pf)          # C's integer division truncates toward zero


def masked_fsc(A_ft, B_ft, n_shell, mask=None, core_radius=None, edge=6, seed=0, method=0):
    """thx_fsc_masked.  Exactly one of ``mask`` (float32 [N, N, N], origin at
    [0, 0, 0]) and ``core_radius`` (> 0, in voxels; ``edge`` is its soft edge,
    the reference's EDGE_WIDTH_RL = 6).  method: as ops.fft3d's.  Returns the
    named tuple (fsc, unmasked, masked, randomised, thres): four float64
    [n_shell] device tensors and t as a Python int (the one read-back, after
    everything is enqueued)."""
    if A_ft.dim() != 3 or A_ft.shape[0] != A_ft.shape[1] or A_ft.shape[2] != A_ft.shape[0] // 2 + 1:
        raise ValueError(f"A_ft: expected [N, N, N/2+1] half-complex, got {tuple(A_ft.shape)}")
    _req(A_ft, torch.complex64, None, "A_ft")
    _req(B_ft, torch.complex64, tuple(A_ft.shape), "B_ft")
    N = A_ft.shape[0]
    dev = A_ft.device
    if (mask is None) == (core_radius is None):
        raise ValueError("masked_fsc: give exactly one of mask and core_radius")
    if mask is not None:
        _req(mask, torch.float32, (N, N, N), "mask")
    out = torch.empty(n_shell, dtype=torch.float64, device=dev)
    curves = torch.empty(3, n_shell, dtype=torch.float64, device=dev)
    t = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        need = lib().thx_fsc_masked_workspace(N, int(n_shell))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)   # large: not kept in the cache
        check(lib().thx_fsc_masked(_ptr(A_ft), _ptr(B_ft), N, int(n_shell), _ptr(mask),
                                   0.0 if core_radius is None else float(core_radius), float(edge),
                                   int(seed), int(method), _ptr(out), _ptr(curves), _ptr(t),
                                   _ptr(ws), need, _stream(dev)), "thx_fsc_masked")
    return MaskedFSC(out, curves[0], curves[1], curves[2], int(t.item()))
