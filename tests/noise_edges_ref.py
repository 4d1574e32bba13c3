"""Float64 restatement of the noise-model kernels (csrc/noise.hip) with
absolute budgets counted from the kernels (test infrastructure, host only).

Composed from what the project already has: the pixel domain is
``noise_ref.domain`` (brute force, never thx_spectrum_pixels); the 3D gather is
``scatter_ref.project_f64`` (float64 trilinear taps on the FP32-rounded
coordinate, with its per-pixel budget), the 2D gather ``twod_ref.project2d_64``
with ``twod_ref.gather_budget``; the CTF and its absolute FP32 error are
``scatter_ref.ctf_f64`` at the defocus pair (float32(dU d), float32(dV d)), as
k_residual forms it.  Everything after the coordinate is float64: the phase
exp(-2 pi i (iCol tx + iRow ty) / N) from the float64 translation (t for M,
t - off for N), M = c P phase, the four terms |img - M|^2, |ori - N|^2, |M|^2,
|img|^2, their shell means and the norm over rL^2 <= i^2 + j^2 < rNorm^2.  The
radii are squared from the float32 values the ABI takes and rounded to float32
as residual_launch does, so a fractional bound decides as the device does.

Budgets, all absolute, u = 2^-24, no floor relative to a shell's or an image's
maximum:

  per pixel   dM <= |c| b_P + |P| dctf + |M| u (K_M + 4 P theta)
    b_P       the gather's budget
    dctf      ctf_f64's bound on the FP32 CTF
    theta     2 pi (|iCol tx| + |iRow ty|) / N: the translation cast to FP32,
              divided by idim, multiplied by iCol and iRow and added, four
              roundings of that magnitude
    P         the phase margin: 1 for libm, 4 for the device (the project's
              rule for every phase_shift output)
    K_M = 7   cmul(P, T) two products and an add per component 3; the hardware
              sin / cos round T once more 1; the product with c 1; the float
              conversion and the division that form mCol, counted once more as
              relative roundings of M, 2
  a term      |e|^2 with e = v - M: 2 |e| dM + dM^2 + K_E u (|e| + dM)^2,
              K_E = 5: forming e rounds both components once (2 u |e|^2), the
              two squares and their add 3
              |M|^2: 2 |M| dM + dM^2 + K_SQ u (|M| + dM)^2, K_SQ = 3
              |img|^2: K_SQ u |img|^2 (no model error)
  a shell     the mean of its terms' budgets plus
              u (ceil(count / 64) + 6 + 1) mean(term + its budget): a lane's
              chain of ceil(count / 64) additions, the six butterfly steps of
              wave_sum and the division by the count.  The order is fixed by
              the table, so this is tighter than count u.
  the norm    an FP64 sum of the FP32 residual terms: the sum of its pixels'
              term budgets.

The accumulate, the rows and the rescale are restated operation by operation
(``accumulate_emu``, ``rows_emu``, ``scale_emu``): halving a float and adding
FP64 in image order is the same arithmetic on host and device, so rows 0, 1
and the counts are compared bit for bit; row 2 (an FP64 division and root per
image) is bounded by (n + 2) 2^-53 sum |t|, n the group's image count.

``mut`` names a deliberately wrong restatement (test_noise_edges_ref.py).
"""
import types

import numpy as np

import noise_ref as NR
import scatter_ref as SC
import twod_ref as T2

U = 2.0 ** -24
K_M = 7
K_E = 5
K_SQ = 3
NA_DEPTH = 8              # k_sigma_accumulate's batch
ROWS_SPAN = 32 * 256      # k_sig_rcp_rows' grid cap times its block
SCALE_SPAN = 64 * 256     # k_img_scale's
SENTINEL = 7.0            # what an unwritten output still holds

MUTS = ("mirror0", "floor", "le_rN", "gt_rL", "drop128", "noconj")


def n_chain(count):
    return -(-np.asarray(count) // 64) + 6 + 1


# -------------------------------------------------------------------- pixels
def pixels(N, r, mut=None):
    """The disc of powerSpectrum in its loop order, with the rank of every
    pixel inside its shell (table order) and the shells' counts."""
    if mut == "floor":         # the shell by floor: (2, 2) joins shell 2 instead of leaving the disc
        a = np.array([(i, j, int(np.floor(np.hypot(i, j))), (j if j >= 0 else j + N) * (N // 2 + 1) + i)
                      for j in range(-N // 2, N // 2) for i in range(N // 2 + 1)
                      if i * i + j * j < r * r], np.int32)
        iCol, iRow, iShell, iPxl = (a[:, k].copy() for k in range(4))
    else:
        iCol, iRow, iShell, iPxl = NR.domain(N, r)
    count = np.bincount(iShell, minlength=r)
    start = np.concatenate([[0], np.cumsum(count)])
    o = np.argsort(iShell, kind="stable")
    rank = np.empty(len(o), np.int64)
    rank[o] = np.arange(len(o)) - start[iShell[o]]
    return types.SimpleNamespace(iCol=iCol, iRow=iRow, iSig=iShell, iPxl=iPxl, n=len(iCol),
                                 count=count, rank=rank, N=N, r=r)


def read(img, px, mut=None):
    """The stored pixels of the disc; column 0 below the axis is read, not
    mirrored from above it."""
    img = np.asarray(img)
    v = img.reshape(-1)[px.iPxl].astype(np.complex128)
    if mut == "mirror0":
        m = (px.iCol == 0) & (px.iRow < 0)
        v[m] = np.conj(img[-px.iRow[m], 0].astype(np.complex128))
    return v


def shell_mean(t, px, mut=None):
    w = np.where(px.rank >= 128, 0.0, t) if mut == "drop128" else t
    return np.bincount(px.iSig, weights=w, minlength=px.r)[:px.r] / px.count[:px.r]


def shell_budget(t, bt, px):
    """mean of the terms' budgets plus the fixed-order FP32 sum and divide"""
    return shell_mean(bt, px) + U * n_chain(px.count[:px.r]) * shell_mean(t + bt, px)


def p2(z):
    return z.real * z.real + z.imag * z.imag


def power_spectrum(img, px, mut=None):
    """(shell means of |img|^2 [n, r], budget [n, r])"""
    out, bud = [], []
    for a in img:
        t = p2(read(a, px, mut))
        out.append(shell_mean(t, px, mut))
        bud.append(shell_budget(t, K_SQ * U * t, px))
    return np.stack(out), np.stack(bud)


# ---------------------------------------------------------------------- model
def mats3(quat):
    return SC._mats(quat)


def fused_agree3(mat, iCol, iRow, pf):
    """twod_ref.fused_agree for rot_coord: the FP32-rounded coordinate and the
    fold decision ``x >= 0`` (to which -0.0 is +0.0) are the same whether
    m[a] nx + m[3 + a] ny rounds each product or is contracted into a fused
    multiply-add (either product)."""
    mat = np.asarray(mat, np.float64).reshape(-1, 9)
    X = (np.asarray(iCol, np.int64) * pf).astype(np.float64)
    Y = (np.asarray(iRow, np.int64) * pf).astype(np.float64)
    ok = np.ones(len(mat), bool)
    for q, m in enumerate(mat):
        for a in range(3):
            pa, pb = m[a] * X, m[3 + a] * Y
            v = pa + pb
            dl = 2.0 ** -51 * (np.abs(pa) + np.abs(pb))
            lo, hi = (v - dl).astype(np.float32), (v + dl).astype(np.float32)
            for i in np.flatnonzero((lo != hi) | (np.signbit(lo) != np.signbit(hi))):
                want = np.float32(v[i])
                for f in T2._fused(m[a], X[i], m[3 + a], Y[i], 1):
                    g = np.float32(f)
                    if g != want or (g >= 0) != (want >= 0):
                        ok[q] = False
    return ok


def coords(case, l, px):
    """image l's sample coordinates as the gather's reference takes them"""
    if case.two_d:
        return T2.coords2_64(case.rot[l], px.iCol, px.iRow, case.pf)
    x, y, z = SC.coords_f32(mats3(case.rot[l]), px.iCol, px.iRow, case.pf)
    return x[0], y[0], z[0]


def gather(case, l, px, mut=None):
    """(P [nPxl] complex128, b_P [nPxl]) of image l's class at its rotation"""
    vol = case.vols[0 if case.cls is None else int(case.cls[l])]
    if case.two_d:
        P, Pa, D, L1 = T2.project2d_64(vol, case.rot[l][None], px.iCol, px.iRow, case.pf,
                                       mut="noconj" if mut == "noconj" else None, extras=True)
        return P[0], T2.gather_budget(Pa[0], D[0], L1[0])
    mat = mats3(case.rot[l])
    P, b = SC.project_f64(vol, case.vdim, case.pf, mat, px)
    if mut == "noconj":
        x = SC.coords_f32(mat, px.iCol, px.iRow, case.pf)[0]
        P = np.where(~(x >= 0), np.conj(P), P)
    return P[0], b[0]


def ctf(case, l, px):
    """(c, dctf) at (float32(dU d), float32(dV d))"""
    a = np.array(case.attr[l], np.float32)
    if case.dF is not None:
        a[2] = np.float32(np.float64(a[2]) * case.dF[l])
        a[3] = np.float32(np.float64(a[3]) * case.dF[l])
    c, dc = SC.ctf_f64(a, [1.0], px.iCol, px.iRow, case.N)
    return c[0], dc[0]


def phase(t, px):
    a, b = px.iCol * float(t[0]), px.iRow * float(t[1])
    return np.exp(-2j * np.pi * (a + b) / px.N), 2 * np.pi * (np.abs(a) + np.abs(b)) / px.N


def models(case, l, px, margin, mut=None):
    """(M, dM, Nn, dN) on the disc for image l"""
    P, bP = gather(case, l, px, mut)
    c, dc = ctf(case, l, px)
    off = np.zeros(2) if case.off is None else case.off[l]
    out = []
    for t in (case.trans[l], case.trans[l] - off):
        T, th = phase(t, px)
        M = c * P * T
        out += [M, np.abs(c) * bP + np.abs(P) * dc + np.abs(M) * U * (K_M + 4 * margin * th)]
    return out


def sq_f32(x):
    """(float)((double)x * x) of a float argument"""
    x = np.float64(np.float32(x))
    return np.float64(np.float32(x * x))


def annulus(px, rL, rN, mut=None):
    quad = (px.iCol.astype(np.int64) ** 2 + px.iRow.astype(np.int64) ** 2).astype(np.float64)
    lo = quad > sq_f32(rL) if mut == "gt_rL" else quad >= sq_f32(rL)
    hi = quad <= sq_f32(rN) if mut == "le_rN" else quad < sq_f32(rN)
    return lo & hi


def residual(case, margin, mut=None, radii=None):
    """spectra [n, 4, r], their budget, and per pair of ``radii`` (default
    case.radii) norm [nPair, n] with its budget."""
    px = pixels(case.N, case.r, mut)
    radii = case.radii if radii is None else radii
    n = len(case.img)
    S, B = np.zeros((n, 4, case.r)), np.zeros((n, 4, case.r))
    nrm, bn = np.zeros((len(radii), n)), np.zeros((len(radii), n))
    for l in range(n):
        M, dM, Nn, dN = models(case, l, px, margin, mut)
        v, o = read(case.img[l], px, mut), read(case.ori[l], px, mut)
        rows = []
        for a, m, d in ((v, M, dM), (o, Nn, dN)):
            e = np.abs(a - m)
            rows.append((p2(a - m), 2 * e * d + d * d + K_E * U * (e + d) ** 2))
        aM = np.abs(M)
        rows.insert(2, (p2(M), 2 * aM * dM + dM * dM + K_SQ * U * (aM + dM) ** 2))
        rows.append((p2(v), K_SQ * U * p2(v)))
        for q, (t, bt) in enumerate(rows):
            S[l, q] = shell_mean(t, px, mut)
            B[l, q] = shell_budget(t, bt, px)
        for k, (rL, rN) in enumerate(radii):
            m = annulus(px, rL, rN, mut)
            nrm[k, l] = rows[0][0][m].sum()
            bn[k, l] = rows[0][1][m].sum()
    return S, B, nrm, bn


def worst(got, ref, bound):
    return T2.worst(got, ref, bound)


# ----------------------------------------------------------------- accumulate
def accumulate_emu(spectra, group, n_group, acc=None, mut=None):
    """k_sigma_accumulate operation by operation: batches of NA_DEPTH images,
    the tail clamped to the last image and selected away, FP64 additions in
    image order.  mut: "last_twice" (the tail's ``in`` without l0 + k < nImg),
    "skip8" (the second trip starts a batch late), "mulzero" (other groups'
    terms multiplied by zero instead of selected)."""
    s = np.asarray(spectra, np.float32)
    n, _, r = s.shape
    acc = np.zeros((3, n_group, r + 1)) if acc is None else np.array(acc, np.float64)
    g_of = np.arange(n_group)[:, None]
    l0 = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while l0 < n:
            for k in range(NA_DEPTH):
                l = min(l0 + k, n - 1)
                gl = 0 if group is None else int(group[l])
                inn = (g_of == gl) & (l0 + k < n or mut == "last_twice")          # [nGroup, 1]
                v = s[l].astype(np.float64)
                terms = (v[0] / 2, v[1] / 2, np.sqrt(v[2] / v[3]))
                for q in range(3):
                    t = np.concatenate([terms[q], [1.0]])[None, :]
                    acc[q] += t * np.where(inn, 1.0, 0.0) if mut == "mulzero" else np.where(inn, t, 0.0)
            l0 += 2 * NA_DEPTH if (mut == "skip8" and l0 == 0) else NA_DEPTH
    return acc


def sigma_sums(spectra, group, n_group):
    with np.errstate(divide="ignore", invalid="ignore"):
        return NR.sigma_sums(np.asarray(spectra, np.float32), group, n_group)


def row2_bound(spectra, group, n_group):
    """(n_g + 2) 2^-53 sum |t| per (group, shell): the division, the root and
    the n_g additions; non-finite where a term is"""
    s = np.asarray(spectra, np.float64)
    n, _, r = s.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.sqrt(s[:, 2] / s[:, 3])
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    tot, cnt = np.zeros((n_group, r)), np.zeros(n_group)
    np.add.at(tot, g, np.abs(t))
    np.add.at(cnt, g, 1)
    return (cnt[:, None] + 2) * 2.0 ** -53 * tot


# ----------------------------------------------------------------- rows, scale
def rows_emu(sig_rcp, group, i_sig, n, mut=None):
    """k_sig_rcp_rows: float32(sigRcp[g, u]), NaN for a group or a column out
    of range.  mut "one_trip": the stride loop as a single ``if``."""
    sig_rcp = np.asarray(sig_rcp, np.float64)
    n_group, n_col = sig_rcp.shape
    i_sig = np.asarray(i_sig, np.int64)
    out = np.full((n, len(i_sig)), SENTINEL, np.float32)
    m = len(i_sig) if mut != "one_trip" else min(len(i_sig), ROWS_SPAN)
    u = i_sig[:m]
    uok = (u >= 0) & (u < n_col)
    for l in range(n):
        g = 0 if group is None else int(group[l])
        row = np.full(m, np.nan, np.float32)
        if 0 <= g < n_group:
            row[uok] = sig_rcp[g, u[uok]].astype(np.float32)
        out[l, :m] = row
    return out


def scale_emu(img, scale, mut=None):
    """k_img_scale: both components times the float scale, in FP32"""
    v = np.array(img, np.complex64)
    f = v.view(np.float32).reshape(len(v), -1, 2)
    m = f.shape[1] if mut != "one_trip" else min(f.shape[1], SCALE_SPAN)
    f[:, :m] *= np.asarray(scale, np.float32)[:, None, None]
    return v


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
