"""Mask generation on the device: THUNDER's ``thunder_genmask`` (genMask /
removeIsolatedPoint / extMask / softEdge, src/Functions/Mask.cpp:581-731, with
the tool's corner removal, appsrc/thunder_genmask.cpp:156-159) over the kernels
of csrc/mask.hip.

    m = mask.gen_mask(vol, thres, ext=4, edge=6)            # the three stages chained
    m = mask.soft_edge(mask.extend(mask.threshold(vol, thres), 4), 6)   # the same, by stage
    mask.save_mask("mask.mrc", m, pixel_size)

Maps are float32 [N, N, N] device tensors with the origin at [0, 0, 0] and
negative coordinates wrapped, as everywhere in this package (the ``alphaMask``
of ``reference.refresh_projectee``, ``subtract`` and ``resolution.masked_fsc``);
N even, 16 <= N <= 1024, |ext| <= 32, edge <= 32.  Nothing wraps at a box face.
``autoMask``'s threshold search is not provided.
"""
import numpy as np
import torch

from . import io
from ._lib import check, lib
from .ops import _ptr, _req, _stream, workspace


def _cube(vol, name="vol"):
    if vol.dim() != 3 or len(set(vol.shape)) != 1:
        raise ValueError(f"{name}: expected [N, N, N], got {tuple(vol.shape)}")
    _req(vol, torch.float32, None, name)
    return vol.shape[0]


def threshold(vol, thres, remove_corners=True):
    """thx_mask_threshold: vol > thres as 0 / 1 (corners i^2 + j^2 + k^2 >=
    (N/2)^2 counting as 0 first), without its isolated points."""
    N = _cube(vol)
    out = torch.empty_like(vol)
    with torch.cuda.device(vol.device):
        check(lib().thx_mask_threshold(_ptr(vol), N, float(thres), int(bool(remove_corners)),
                                       _ptr(out), _stream(vol.device)), "thx_mask_threshold")
    return out


def _staged(fn, name, m, value):
    N = _cube(m, "mask")
    out = torch.empty_like(m)
    with torch.cuda.device(m.device):
        ws = workspace(lib().thx_gen_mask_workspace(N), m.device)
        check(fn(_ptr(m), N, float(value), _ptr(out), _ptr(ws), ws.numel(), _stream(m.device)), name)
    return out


def extend(m, ext):
    """thx_mask_extend: extMask.  ext > 0 grows the 1-voxels by the open ball
    |d|^2 < ext^2, ext < 0 grows the 0-voxels inside the box, 0 copies."""
    return _staged(lib().thx_mask_extend, "thx_mask_extend", m, ext)


def soft_edge(m, edge):
    """thx_mask_soft_edge: softEdge.  A voxel at distance 0 < d < edge of a
    1-voxel becomes 0.5 + 0.5 cos(d / edge pi); edge <= 0 copies."""
    return _staged(lib().thx_mask_soft_edge, "thx_mask_soft_edge", m, edge)


def gen_mask(vol, thres, ext, edge, remove_corners=True):
    """thx_gen_mask: threshold, extend and soft edge chained on the stream
    (what thunder_genmask computes with remove_corners)."""
    N = _cube(vol)
    out = torch.empty_like(vol)
    with torch.cuda.device(vol.device):
        ws = workspace(lib().thx_gen_mask_workspace(N), vol.device)
        check(lib().thx_gen_mask(_ptr(vol), N, float(thres), float(ext), float(edge),
                                 int(bool(remove_corners)), _ptr(out), _ptr(ws), ws.numel(),
                                 _stream(vol.device)), "thx_gen_mask")
    return out


def save_mask(path, mask, pixel_size):
    """Write a mask (tensor or array [N, N, N], origin at [0, 0, 0]) as an MRC
    map in the centred layout thunder_genmask writes (ImageFile::writeVolume:
    the origin moves to [N/2, N/2, N/2])."""
    a = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
    if a.ndim != 3 or len(set(a.shape)) != 1:
        raise ValueError(f"mask: expected [N, N, N], got {a.shape}")
    io.write_mrc(path, np.fft.fftshift(a.astype(np.float32)), pixel_size)
    return path
