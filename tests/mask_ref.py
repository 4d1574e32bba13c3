"""numpy restatement of THUNDER's mask generation (src/Functions/Mask.cpp:
581-731, appsrc/thunder_genmask.cpp:156-159), written independently of
csrc/mask.hip and in the reference's own scatter form: every source voxel
writes the grid [-a, a)^3 around itself, a = ceil(radius), under the
reference's tests in its types (QUAD_3 as a double against the RFLOAT square;
RFLOAT(NORM_3) against the RFLOAT edge width).  A write outside the box is
dropped (the reference indexes linearly without bounds checks there, which is
an out-of-row write, not behaviour to restate).

Maps are [N, N, N] with the origin at index 0 and negatives wrapped; the work is
done on the centred map (np.fft.fftshift: index p = i + N/2), where a box face
is an array edge.  A plain module: import it from a test.
"""
import math

import numpy as np

FLT_MAX = np.finfo(np.float32).max
FORCE_ORDER = None          # "offsets" / "sources": pin _scatter's loop order (its own test)


def threshold(src, thres, remove_corners=True):
    """genMask(dst, src, thres) after thunder_genmask's corner removal."""
    c = np.fft.fftshift(np.asarray(src, np.float32)).copy()
    N = c.shape[0]
    ax = np.arange(N) - N // 2
    k, j, i = np.meshgrid(ax, ax, ax, indexing="ij")
    if remove_corners:
        c[i * i + j * j + k * k >= (N // 2) ** 2] = 0
    m = np.where(c > np.float32(thres), np.float32(1), np.float32(0))
    # removeIsolatedPoint: the six face neighbours inside the box, on the copy
    p = np.pad(m, 1)
    near = ((p[:-2, 1:-1, 1:-1] == 1) | (p[2:, 1:-1, 1:-1] == 1) | (p[1:-1, :-2, 1:-1] == 1) |
            (p[1:-1, 2:, 1:-1] == 1) | (p[1:-1, 1:-1, :-2] == 1) | (p[1:-1, 1:-1, 2:] == 1))
    out = m.copy()
    out[(m == 1) & ~near] = 0
    return np.fft.ifftshift(out)


def _grid(a):
    """offsets of VOLUME_FOR_EACH_PIXEL_IN_GRID(a): [-a, a)^3 as z, y, x arrays"""
    g = np.arange(-a, a)
    return np.meshgrid(g, g, g, indexing="ij")


def _clip(p, a, N):
    """source voxel p, grid [-a, a): (box slice, grid slice) of what stays in the box"""
    lo, hi = max(p - a, 0), min(p + a, N)
    return slice(lo, hi), slice(lo - (p - a), hi - (p - a))


def _scatter(sel, keep, apply_offset, apply_source, a):
    """Run the scatter of the selected source voxels over the grid offsets that
    pass (keep [2a, 2a, 2a] bool) in whichever loop order is cheaper: offsets
    outside (one shifted whole-map write per offset) or sources outside (one
    clipped grid write per source).  Both visit the same (source, offset) set."""
    N = sel.shape[0]
    n_src, n_off = int(sel.sum()), int(keep.sum())
    by_offsets = n_off * (N ** 3) * 2.5e-9 <= n_src * (8e-6 + min(n_off, N ** 3) * 2e-9)
    if FORCE_ORDER is not None:
        by_offsets = FORCE_ORDER == "offsets"
    if by_offsets:
        zs, ys, xs = np.nonzero(keep)
        for z, y, x in zip(zs - a, ys - a, xs - a):
            d, s = [], []
            for o in (z, y, x):
                d.append(slice(max(o, 0), N + min(o, 0)))       # destination = source + offset
                s.append(slice(max(-o, 0), N + min(-o, 0)))
            if all(t.start < t.stop for t in d):
                apply_offset(tuple(d), tuple(s), (int(z), int(y), int(x)))
    else:
        for pz, py, px in zip(*np.nonzero(sel)):
            (bz, gz), (by, gy), (bx, gx) = _clip(pz, a, N), _clip(py, a, N), _clip(px, a, N)
            apply_source((bz, by, bx), (gz, gy, gx))


def extend(m, ext):
    """extMask"""
    m = np.asarray(m, np.float32)
    ext = np.float32(ext)
    if ext == 0:
        return m.copy()
    c = np.fft.fftshift(m)
    out = c.copy()
    a = int(math.ceil(abs(float(ext))))
    e2 = float(np.float32(float(ext) * float(ext)))          # TSGSL_pow_2: RFLOAT
    z, y, x = _grid(a)
    keep = (x * x + y * y + z * z).astype(np.float64) < e2    # QUAD_3: double
    sel = c == 1 if ext > 0 else c == 0
    val = np.float32(1 if ext > 0 else 0)

    def by_offset(d, s, _):
        out[d][sel[s]] = val

    def by_source(box, grid):
        out[box][keep[grid]] = val
    _scatter(sel, keep, by_offset, by_source, a)
    return np.fft.ifftshift(out)


def soft_edge(m, ew):
    """softEdge"""
    m = np.asarray(m, np.float32)
    ew = np.float32(ew)
    if not ew > 0:
        return m.copy()
    c = np.fft.fftshift(m)
    a = int(math.ceil(float(ew)))
    z, y, x = _grid(a)
    dist_of = np.sqrt((x * x + y * y + z * z).astype(np.float64)).astype(np.float32)   # RFLOAT d
    keep = dist_of < ew
    ball = np.where(keep, dist_of, FLT_MAX).astype(np.float32)
    distance = np.full(c.shape, FLT_MAX, np.float32)
    sel = c == 1

    def by_offset(d, s, off):
        dv = dist_of[off[0] + a, off[1] + a, off[2] + a]
        view = distance[d]
        view[sel[s] & (view > dv)] = dv

    def by_source(box, grid):
        np.minimum(distance[box], ball[grid], out=distance[box])
    _scatter(sel, keep, by_offset, by_source, a)
    out = c.copy()
    hit = (distance != 0) & (distance < ew)
    d = distance[hit]
    out[hit] = (0.5 + 0.5 * np.cos((d / ew).astype(np.float64) * math.pi)).astype(np.float32)
    return np.fft.ifftshift(out)


def gen_mask(src, thres, ext, ew, remove_corners=True):
    """genMask(dst, src, thres, ext, ew) after the corner removal"""
    return soft_edge(extend(threshold(src, thres, remove_corners), ext), ew)
