"""The map tools on the device: THUNDER's ``thunder_alignZ``, ``thunder_resize``,
``thunder_project``, ``thunder_mask``, ``thunder_average`` and ``thunder_minus``
and the real-space symmetrisation (SYMMETRIZE_RL), over the kernels of
csrc/maptools.hip.

    v = maptools.align_z(vol, (1, 1, 0))               # a symmetry axis onto z
    v = maptools.symmetrize(vol, "C4")                 # vol plus its rotated copies
    v = maptools.resize(vol, 128)                      # Fourier crop / pad
    img = maptools.project(projectee, quat, N)         # real-space projections [n, N, N]
    maptools.run_resize("in.mrc", "out.mrc", 128, 1.32)    # the tools: MRC in, MRC out

Maps are as everywhere in this package: real float32 [N, N, N] device tensors
with the origin at [0, 0, 0] and negative coordinates wrapped, transforms
complex64 [N, N, N/2+1] unnormalised; N even, 16 <= N <= 1024.  MRC files are
centred (fftshift on write, ifftshift on read).  Every call is stream-ordered
and bit-identical from run to run.

``resize`` does not renormalise, as the reference does not: the mean of the
result is (N/M)^3 times the input's.
"""
import math

import numpy as np
import torch

from . import io, ops, reference
from ._lib import check, lib
from .ops import _ptr, _req, _stream

EDGE_WIDTH_RL = 6.0             # pixels (include/Config.h)
EQUAL_ACCURACY = 1e-2           # alignZ's test for a vector along x
_INTERP = {"nearest": 0, "linear": 1}


def _cube(vol, name="vol"):
    if vol.dim() != 3 or len(set(vol.shape)) != 1:
        raise ValueError(f"{name}: expected [N, N, N], got {tuple(vol.shape)}")
    _req(vol, torch.float32, None, name)
    return vol.shape[0]


def _half_complex(ft, name="ft"):
    if ft.dim() != 3 or ft.shape[0] != ft.shape[1] or ft.shape[2] != ft.shape[0] // 2 + 1:
        raise ValueError(f"{name}: expected [N, N, N/2+1] half-complex, got {tuple(ft.shape)}")
    _req(ft, torch.complex64, None, name)
    return ft.shape[0]


def _box(M, name="M"):
    M = int(M)
    if M % 2 or not 16 <= M <= 1024:
        raise ValueError(f"{name}={M}: must be even, in [16, 1024]")
    return M


def _mats(mats, device):
    """[n, 3, 3] / [3, 3] / [n, 9] (numpy or tensor) -> float64 [n, 9] on device"""
    m = mats if torch.is_tensor(mats) else torch.as_tensor(np.asarray(mats, np.float64))
    if m.numel() == 0:
        return torch.empty(0, 9, dtype=torch.float64, device=device)
    if m.numel() % 9 or m.shape[-1] not in (3, 9):
        raise ValueError(f"mats: expected [n, 3, 3], got {tuple(m.shape)}")
    return m.to(device=device, dtype=torch.float64).reshape(-1, 9).contiguous()


def transform(vol, mats, r=None, interp="linear", add_src=False):
    """thx_vol_transform_rl: out(x) = (add_src ? vol(x) : 0) + sum_m [|M_m x|^2 <
    r^2] interp(vol, M_m x) over the signed voxels x = (i, j, k); mats [n, 3, 3]
    row-major (x' = M x with x = (column, row, slice)), added in index order.
    r defaults to N/2 - 1, the largest radius whose taps stay inside the box.
    VOL_TRANSFORM_MAT_RL with one matrix, SYMMETRIZE_RL with a group's
    elements and add_src."""
    N = _cube(vol)
    if interp not in _INTERP:
        raise ValueError(f"interp: one of {sorted(_INTERP)}")
    r = float(N // 2 - 1 if r is None else r)
    if not 0 < r <= N // 2 - 1:
        raise ValueError(f"r={r}: outside (0, N/2 - 1]")
    m = _mats(mats, vol.device)
    out = torch.empty_like(vol)
    with torch.cuda.device(vol.device):
        check(lib().thx_vol_transform_rl(_ptr(vol), N, _ptr(m) if len(m) else None, len(m), r,
                                         _INTERP[interp], int(bool(add_src)), _ptr(out),
                                         _stream(vol.device)), "thx_vol_transform_rl")
    return out


def align_z_matrix(v):
    """alignZ (src/Geometry/Euler.cpp:239-270) in host float64: the matrix whose
    third row is v / |v|.  For a unit v it is the rotation that takes v to
    (0, 0, 1); a v within EQUAL_ACCURACY of the x axis takes the reference's
    fixed matrix (x -> z, z -> -x).  For any other length the first row, (pYZ,
    -xy/pYZ, -xz/pYZ), is scaled by |v| and the matrix is no rotation."""
    v = np.asarray(v, np.float64).reshape(3)
    x, y, z = (float(c) for c in v)
    p_yz, p = math.sqrt(y * y + z * z), math.sqrt(x * x + y * y + z * z)
    if not p > 0 or not math.isfinite(p):
        raise ValueError("v: must be finite and non-zero")
    if p_yz / p > EQUAL_ACCURACY:
        return np.array([[p_yz, -x * y / p_yz, -x * z / p_yz], [0.0, z / p_yz, -y / p_yz],
                         [x / p, y / p, z / p]])
    return np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])


def align_z(vol, v):
    """thunder_alignZ (appsrc/thunder_alignZ.cpp:158-162): transform(vol,
    alignZ(v), N/2 - 1, linear).  v is normalised first: for a unit vector that
    is the reference exactly; for any other length the reference's matrix is
    not a rotation (see align_z_matrix) and its output is a sheared map, which
    is not reproduced."""
    v = np.asarray(v, np.float64).reshape(3)
    n = float(np.linalg.norm(v))
    if not n > 0 or not math.isfinite(n):
        raise ValueError("v: must be finite and non-zero")
    return transform(vol, align_z_matrix(v / n)[None])


def symmetrize(vol, sym, r=None):
    """SYMMETRIZE_RL (include/Geometry/Transformation.h:139-163): vol plus its
    copies under the non-identity elements of point group ``sym`` (ops.symmetry),
    not divided by the group order, as there."""
    R, _ = ops.symmetry(sym)
    return transform(vol, R, r, "linear", add_src=True)


def ft_resize(ft, M):
    """thx_ft_resize: the half-complex map moved into box M, cropped or zero
    padded at the common cube 0 <= i <= L/2, -L/2 <= j, k < L/2, L = min(N, M)."""
    M = _box(M)
    N = _half_complex(ft)
    out = torch.empty(M, M, M // 2 + 1, dtype=torch.complex64, device=ft.device)
    with torch.cuda.device(ft.device):
        check(lib().thx_ft_resize(_ptr(ft), N, _ptr(out), M, _stream(ft.device)), "thx_ft_resize")
    return out


def resize(vol, M):
    """thunder_resize: fw, ft_resize, bw.  Not renormalised: the mean of the
    result is (N/M)^3 times the input's, as in the reference."""
    M = _box(M)
    N = _cube(vol)
    out = torch.empty(M, M, M, dtype=torch.float32, device=vol.device)
    with torch.cuda.device(vol.device):
        need = lib().thx_vol_resize_workspace(N, M)
        if need == 0:
            raise ValueError(f"resize: N={N} is not supported")
        ws = torch.empty(need, dtype=torch.uint8, device=vol.device)    # large: not kept in the cache
        check(lib().thx_vol_resize(_ptr(vol), N, _ptr(out), M, _ptr(ws), need, _stream(vol.device)),
              "thx_vol_resize")
    return out


def project(projectee, quat_or_mat, N, pf=2, r=None, trans=None, real=True, ft=False, centred=False):
    """thx_project_images: Projector::project(Image&, mat) for n rotations and
    FFT::bw of each.  projectee: complex64 [pf N, pf N, pf N/2+1]
    (reference.refresh_projectee); quat_or_mat: float64 [n, 4] unit quaternions
    or [n, 9] matrices as ops.rotmat writes them; trans: float64 [n, 2], the
    projection then carries the phase ramp of that shift, so one at a particle's
    top pose overlays its image.  r defaults to N/2 - 1 (setProjectee's
    _maxRadius).  Returns the real images float32 [n, N, N] (``centred``: the
    layout of an MRC stack), the transforms complex64 [n, N, N/2+1], or (real,
    transforms) with both flags."""
    vdim = ops._vol_dim(projectee)
    N = _box(N, "N")
    if vdim != pf * N:
        raise ValueError(f"projectee: box {vdim}, expected pf N = {pf * N}")
    if not (real or ft):
        raise ValueError("project: neither real nor ft is wanted")
    r = N // 2 - 1 if r is None else int(r)
    if not 1 <= r <= N // 2 - 1:
        raise ValueError(f"r={r}: outside [1, N/2 - 1]")
    dev = projectee.device
    q = quat_or_mat
    n = q.shape[0]
    if q.dim() != 2 or q.shape[1] not in (4, 9):
        raise ValueError(f"quat_or_mat: expected [n, 4] or [n, 9], got {tuple(q.shape)}")
    _req(q, torch.float64, None, "quat_or_mat")
    mat = ops.rotmat(q) if q.shape[1] == 4 and n else q
    if trans is not None:
        _req(trans, torch.float64, (n, 2), "trans")
    img_ft = torch.empty(n, N, N // 2 + 1, dtype=torch.complex64, device=dev) if ft else None
    img_rl = torch.empty(n, N, N, dtype=torch.float32, device=dev) if real else None
    if n:
        with torch.cuda.device(dev):
            need = lib().thx_project_images_workspace(n, N) if real else 0
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
            check(lib().thx_project_images(_ptr(projectee), vdim, pf, _ptr(mat), _ptr(trans), n, N, r,
                                           _ptr(img_ft), _ptr(img_rl), int(bool(centred)), _ptr(ws),
                                           need, _stream(dev)), "thx_project_images")
    return (img_rl, img_ft) if real and ft else img_rl if real else img_ft


def soft_mask(vol, r, edge=EDGE_WIDTH_RL, out=None):
    """thx_vol_soft_mask: softMask(dst, src, r, edge, bg = 0), thunder_mask's
    radial mask; ``out`` may be vol itself."""
    N = _cube(vol)
    out = torch.empty_like(vol) if out is None else _req(out, torch.float32, (N, N, N), "out")
    with torch.cuda.device(vol.device):
        check(lib().thx_vol_soft_mask(_ptr(vol), N, float(r), float(edge), _ptr(out),
                                      _stream(vol.device)), "thx_vol_soft_mask")
    return out


def average(a, b):
    """thunder_average: (a + b) / 2, in that order"""
    _pair(a, b)
    return (a + b) / 2


def minus(a, b):
    """thunder_minus: a - b"""
    _pair(a, b)
    return a - b


def _pair(a, b):
    """two maps of one box on one device"""
    N = _cube(a, "a")
    _req(b, torch.float32, (N, N, N), "b")
    if b.device != a.device:
        raise ValueError("b: on another device")


# ------------------------------------------------------------------ the tools
def _read(path, device):
    """an MRC map (centred layout) -> float32 [N, N, N] with the origin at [0, 0, 0]"""
    v = np.asarray(io.read_mrc(path)[1], np.float32)
    if v.ndim != 3 or len(set(v.shape)) != 1:
        raise ValueError(f"{path}: a map of shape {v.shape} is not cubic")
    return torch.as_tensor(np.fft.ifftshift(v).copy(), device=torch.device(device))


def _write(path, vol, pixel_size):
    io.write_mrc(path, np.fft.fftshift(vol.cpu().numpy()), pixel_size)
    return vol


def run_resize(input, output, boxsize, pixel_size, device="cuda:0"):
    """thunder_resize -i input -o output --boxsize --pixelsize"""
    return _write(output, resize(_read(input, device), boxsize), pixel_size)


def run_align_z(input, output, v, pixel_size, device="cuda:0"):
    """thunder_alignZ -i input -o output -x -y -z --pixelsize"""
    return _write(output, align_z(_read(input, device), v), pixel_size)


def run_mask(input, output, radius, pixel_size, edge=EDGE_WIDTH_RL, device="cuda:0"):
    """thunder_mask: the radial soft mask of ``radius`` pixels"""
    return _write(output, soft_mask(_read(input, device), radius, edge), pixel_size)


def run_average(input_a, input_b, output, pixel_size, device="cuda:0"):
    """thunder_average"""
    return _write(output, average(_read(input_a, device), _read(input_b, device)), pixel_size)


def run_minus(input_a, input_b, output, pixel_size, device="cuda:0"):
    """thunder_minus"""
    return _write(output, minus(_read(input_a, device), _read(input_b, device)), pixel_size)


def run_project(input, output, metadata, n, pixel_size, seed, rank=0, world=1, chunk=None,
                device="cuda:0"):
    """thunder_project (appsrc/thunder_project.cpp:145-234): n projections of
    the map at uniform random orientations, n rounded down to a multiple of
    ``world``; this rank writes its n / world images to <output>_Rank_%06d.mrcs
    (centred, ``chunk`` images per call) and one metadata line per image,
    "%012d@<output>_Rank_%06d.mrcs q0 q1 q2 q3"; rank 0 creates the metadata
    file, the others append, so run the ranks in order.  The quaternions are the
    package's Philox stream under ``seed`` (thx_global_sample_set), the same on
    every rank; the reference draws sampleACG(1, 1, 1, n) from GSL, so the two
    agree in distribution only, and the metadata holds what was projected.
    Returns (stack path, quaternions of this rank as float64 numpy [n / world, 4])."""
    n, world, rank = int(n), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank={rank}, world={world}: need 0 <= rank < world")
    if n < 0:
        raise ValueError(f"n={n}: is negative")
    n = n // world * world
    each = n // world
    vol = _read(input, device)
    N = vol.shape[0]
    proj = reference.refresh_projectee(vol, pf=2)           # setProjectee: no mask
    if n:
        quat = ops.global_sample_set(n, 2, 1.0, int(seed), vol.device)[0]
    else:
        quat = torch.empty(0, 4, dtype=torch.float64, device=vol.device)
    mine = quat[rank * each:(rank + 1) * each].contiguous()
    chunk = max(1, each if chunk is None else int(chunk))
    stack = "%s_Rank_%06d.mrcs" % (output, rank)
    imgs = np.empty((each, N, N), np.float32)
    for c0 in range(0, each, chunk):
        imgs[c0:c0 + chunk] = project(proj, mine[c0:c0 + chunk], N, centred=True).cpu().numpy()
    if each:
        io.write_mrc(stack, imgs, pixel_size)
    q = mine.cpu().numpy()
    with open(metadata, "w" if rank == 0 else "a") as fh:
        for l in range(each):
            fh.write("%012d@%s %18.9f %18.9f %18.9f %18.9f\n" % (l, stack, *q[l]))
    return stack, q
