"""Signal subtraction after the last round: THUNDER's ``Subtract`` option
(Optimiser::run, src/Optimiser.cpp:4163-4363; saveSubtract, :8418-8537; the
subtract branch of saveDatabase, :8295-8361) over the kernels of
csrc/subtract.hip.  3D only, as the reference.

    centre = subtract.region_centroid(region_map)          # _regionCentre (:4180-4211)
    out = subtract.subtract(vol, stack.oriFT, stack.attr, quat, trans, r,
                            offS=off, cls=cls, sym="C2", centre=centre)
    subtract.write_subtract(prefix, out.diffRL.cpu().numpy(), out.quat.cpu().numpy(),
                            stack.attr.cpu().numpy(), pixel_size=stack.pixel_size)
    # or both, in image chunks:
    subtract.save_subtract(stack, vol, quat, trans, r, prefix, sym="C2", centre=centre)

Pose source: one pose per image from the caller (quat [n, 4], trans [n, 2],
dF [n], cls [n]), as in noise.py; the reference takes Particle::rank1st,
which ``Expectation.rank1st()`` returns.

The reference's flow around the subtraction (:4220-4330) is two passes, and
the caller follows it with the calls this package already has -- there is no
orchestrator for it here:

  1. the final reference: ``reference.average_halves`` on the two hemispheres'
     maps;
  2. the unmasked pass: ``reference.refresh_projectee(ref, mask=None)``, then
     ``NoiseModel.norm_correction`` against that projectee, and one more
     reconstruction of the rescaled images up to Nyquist;
  3. the masked pass: ``reference.average_halves`` again, then
     ``reference.refresh_projectee(ref, mask=region_mask)`` -- the projectee
     ``vol`` that ``subtract`` renders; the region centre is the centroid of
     the caller's ``regionCentre`` volume, 0 without one (:4180-4211);
  4. ``subtract`` / ``save_subtract``; the caller then takes ``shift`` off its
     particles' translations (:8512-8517).
"""
import os
import types

import numpy as np
import torch

from . import io
from ._lib import check, lib
from .ops import _ptr, _req, _stream, symmetry, workspace

STACK_NAME = "Subtract_Rank_%06d.mrcs"
TABLE_NAME = "Meta_Subtract.thu"


def region_centroid(mask):
    """thx_region_centroid: centroid(const Volume&) (src/Image/ImageFunctions.
    cpp:37-62) of a real map float32 [N, N, N] (origin at [0, 0, 0], negatives
    wrapped) -> [3] float64 on the device, (i, j, k) order.  A map that sums to
    zero gives inf / NaN, as in the reference."""
    if mask.dim() != 3 or len(set(mask.shape)) != 1:
        raise ValueError(f"mask: expected [N, N, N], got {tuple(mask.shape)}")
    _req(mask, torch.float32, None, "mask")
    N = mask.shape[0]
    dev = mask.device
    out = torch.empty(3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib().thx_region_centroid_workspace(N), dev)
        check(lib().thx_region_centroid(_ptr(mask), N, _ptr(out), _ptr(ws), ws.numel(), _stream(dev)),
              "thx_region_centroid")
    return out


def _sym_matrices(sym, device):
    """[n, 9] float64 on the device (None for no element) from a point-group
    name or an [n, 3, 3] array / tensor"""
    if sym is None:
        return None
    if isinstance(sym, str):
        sym = symmetry(sym)[0]
    R = (sym.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(sym)
         else np.asarray(sym, np.float64))
    if R.size == 0:
        return None
    if R.ndim != 3 or R.shape[1:] != (3, 3):
        raise ValueError(f"sym: expected [n, 3, 3], got {R.shape}")
    return torch.as_tensor(np.ascontiguousarray(R.reshape(-1, 9)), device=device)


def subtract(vol, oriFT, attr, quat, trans, r, pf=2, offS=None, dF=None, cls=None, sym=None,
             centre=None, real=True, model=False, ft=True, centred=True):
    """thx_subtract.  vol: complex64 [nK, vdim, vdim, vdim/2+1] (or one volume),
    the masked reference's projectee; oriFT complex64 [n, N, N/2+1]; attr
    float32 [n, 8]; quat float64 [n, 4]; trans, offS float64 [n, 2]; dF float64
    [n] (None: the unscaled attributes, the reference's behaviour); cls int32
    [n]; sym: a point-group name ("C2", "D2", "I1", ..) or the [nSym, 3, 3]
    non-identity matrices; centre: [3] float64 device tensor (region_centroid)
    or three numbers.

    Returns a namespace of device tensors, copy-major ([1 + nSym, n, ...]):
    diffFT (ft), modelFT (model), diffRL (real; ``centred``: the layout of an MRC
    stack, else the reference's corner origin), quat [1 + nSym, n, 4] (the
    poses saveDatabase writes), shift [n, 2] (= trans - offS), n_sym."""
    if oriFT.dim() != 3 or oriFT.shape[2] != oriFT.shape[1] // 2 + 1:
        raise ValueError(f"oriFT: expected [n, N, N/2+1] half-complex, got {tuple(oriFT.shape)}")
    _req(oriFT, torch.complex64, None, "oriFT")
    n, N = oriFT.shape[0], oriFT.shape[1]
    dev = oriFT.device
    _req(vol, torch.complex64, None, "vol")
    if vol.dim() == 3:
        vol = vol.unsqueeze(0)
    vdim = vol.shape[1]
    if tuple(vol.shape) != (vol.shape[0], vdim, vdim, vdim // 2 + 1):
        raise ValueError(f"vol: expected [nK, vdim, vdim, vdim/2+1], got {tuple(vol.shape)}")
    _req(attr, torch.float32, (n, 8), "attr")
    _req(quat, torch.float64, (n, 4), "quat")
    _req(trans, torch.float64, (n, 2), "trans")
    if offS is not None:
        _req(offS, torch.float64, (n, 2), "offS")
    if dF is not None:
        _req(dF, torch.float64, (n,), "dF")
    if cls is not None:
        _req(cls, torch.int32, (n,), "cls")
    symR = _sym_matrices(sym, dev)
    n_sym = 0 if symR is None else symR.shape[0]
    if centre is not None:
        centre = (centre.to(dev, torch.float64) if torch.is_tensor(centre)
                  else torch.as_tensor(np.asarray(centre, np.float64), device=dev)).contiguous()
        _req(centre, torch.float64, (3,), "centre")
    nc = N // 2 + 1
    copies = 1 + n_sym

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)
    out = types.SimpleNamespace(n_sym=n_sym)
    out.diffFT = new((copies, n, N, nc), torch.complex64) if ft else None
    out.modelFT = new((copies, n, N, nc), torch.complex64) if model else None
    out.diffRL = new((copies, n, N, N), torch.float32) if real else None
    out.quat = new((copies, n, 4), torch.float64)
    out.shift = new((n, 2), torch.float64)
    with torch.cuda.device(dev):
        need = lib().thx_subtract_workspace(n, N, n_sym, int(real))
        ws = new((need,), torch.uint8) if need else None      # large: not kept in the cache
        check(lib().thx_subtract(_ptr(vol), vdim, pf, vol.shape[0], _ptr(oriFT), _ptr(attr),
                                 _ptr(quat), _ptr(trans), _ptr(offS), _ptr(dF), _ptr(cls), n, N,
                                 int(r), _ptr(symR), n_sym, _ptr(centre), _ptr(out.diffFT),
                                 _ptr(out.modelFT), _ptr(out.diffRL), int(bool(centred)),
                                 _ptr(out.quat), _ptr(out.shift), _ptr(ws), need, _stream(dev)),
              "thx_subtract")
    return out


def write_subtract(prefix, diffRL, quat, attr, group=None, cls=None, dF=None, rank=0,
                   pixel_size=None):
    """The host side of saveSubtract / saveDatabase(subtract): no GPU needed.

    diffRL: numpy [1 + nSym, n, N, N] (or flat [(1 + nSym) n, N, N], copy-major)
    as it goes to disk; quat [1 + nSym, n, 4]; attr [n, 8] {pixelSize, voltage,
    dU, dV, theta, Cs, ampContrast, phaseShift}; group, cls [n] (None: 0), dF
    [n] (None: 1).  Writes ``prefix + "Subtract_Rank_%06d.mrcs" % rank`` with
    plane s n + l for copy s of image l, and ``prefix + "Meta_Subtract.thu"``
    with one row per (image, copy) -- image outer, copy inner, as :8287-8360 --
    whose particle path is "%012d@Subtract_Rank_%06d.mrcs" with the 1-based
    plane index, whose quaternion is quat[s, l] and whose translation is 0 (the
    images are recentred: tran - offset is 0 after :8512-8517).  ``prefix`` is
    prepended as a string, like the reference's dstPrefix.  Returns (stack
    path, table path)."""
    quat = np.asarray(quat, np.float64)
    if quat.ndim != 3 or quat.shape[2] != 4:
        raise ValueError(f"quat: expected [1 + nSym, n, 4], got {quat.shape}")
    copies, n = quat.shape[:2]
    d = np.asarray(diffRL)
    if d.ndim == 4:
        d = d.reshape(-1, *d.shape[2:])
    if d.ndim != 3 or d.shape[0] != copies * n or d.shape[1] != d.shape[2]:
        raise ValueError(f"diffRL: expected {copies * n} square planes, got {d.shape}")
    attr = np.asarray(attr, np.float64)
    if attr.shape != (n, 8):
        raise ValueError(f"attr: expected ({n}, 8), got {attr.shape}")
    if pixel_size is None:
        pixel_size = float(attr[0, 0]) if n else 1.0
    stack_name = STACK_NAME % rank
    stack_path, table_path = prefix + stack_name, prefix + TABLE_NAME
    os.makedirs(os.path.dirname(prefix) or ".", exist_ok=True)
    io.write_mrc(stack_path, d, pixel_size)
    l, s = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(copies), indexing="ij"))
    paths = ["%012d@%s" % (li + n * si + 1, stack_name) for li, si in zip(l, s)]
    table = io.thu_table(n * copies, paths, attr[l, 1:8], quat[s, l], None,
                         None if group is None else np.asarray(group)[l])
    if cls is not None:
        table["classID"] = np.asarray(cls, np.int64)[l]
    if dF is not None:
        table["defocusFactor"] = np.asarray(dF, np.float64)[l]
    io.write_thu(table_path, table)
    return stack_path, table_path


def save_subtract(stack, vol, quat, trans, r, prefix, pf=2, offS=None, dF=None, cls=None, sym=None,
                  centre=None, group=None, rank=0, chunk=None):
    """saveSubtract + saveDatabase(subtract) for a whole stack (ingest.Stack
    with keep_ori, or anything with oriFT, attr, pixel_size): subtract in
    chunks of ``chunk`` images (None: about 4096 output planes a call), the
    real-space planes collected on the host in the stack's order, then
    write_subtract.  Returns (stack path, table path, shift [n, 2] float64 on
    the device)."""
    if stack.oriFT is None:
        raise ValueError("save_subtract needs the unmasked oriFT (Stack(keep_ori=True))")
    n, N = stack.oriFT.shape[0], stack.oriFT.shape[1]
    symR = _sym_matrices(sym, stack.oriFT.device)
    copies = 1 + (0 if symR is None else symR.shape[0])
    sym_arg = None if symR is None else symR.view(-1, 3, 3)
    if chunk is None:
        chunk = max(1, 4096 // copies)
    rl = np.empty((copies, n, N, N), np.float32)
    q_out = np.empty((copies, n, 4), np.float64)
    shift = torch.empty(n, 2, dtype=torch.float64, device=stack.oriFT.device)

    def part(t, a, b):
        return None if t is None else t[a:b].contiguous()
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        o = subtract(vol, stack.oriFT[a:b].contiguous(), stack.attr[a:b].contiguous(),
                     part(quat, a, b), part(trans, a, b), r, pf, part(offS, a, b), part(dF, a, b),
                     part(cls, a, b), sym_arg, centre, real=True, model=False, ft=False)
        rl[:, a:b] = o.diffRL.cpu().numpy()
        q_out[:, a:b] = o.quat.cpu().numpy()
        shift[a:b] = o.shift

    def host(t):
        return None if t is None else (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
    sp, tp = write_subtract(prefix, rl, q_out, host(stack.attr), host(group), host(cls), host(dF),
                            rank, getattr(stack, "pixel_size", None))
    return sp, tp, shift
