"""Float64 reference of the global scan and its per-sample error budget.

Pure numpy; takes the FP32 arrays exactly as thx_global_scan gets them:
rotP [nR, nPxl] and traP [nT, nPxl] complex64, dat [nImg, nPxl] complex64,
ctf and sig (sigRcp) [nImg, nPxl] float32, pR [nR] and pT [nT] float64.
sigRcp may carry either sign (the product's is -1 / (2 sigma^2)); every
magnitude sum below takes |s|.

The budget ("The global scan's per-sample budget"), with
u = 2^-24 and per sample
    S_A = sum |s| |d|^2,  S_B = sum |s| c^2 |P|^2 |T|^2,
    S_X = sum 2 |s| |c| |d| |P| |T|,  S = S_A + S_B + S_X
      = sum |s| (|d| + |c| |T P|)^2,
is absolute (no floor relative to |dvp|):
    expanded form   u S (nPxl + K_EXP) + 2^-23 S_B + eps S_X
    direct form     u S (nPxl + K_DIR)
K_EXP and K_DIR count the roundings that form ONE term of the sum, in units
of u times that term's share of S; the accumulation of the nPxl terms, in any
order, is the nPxl u S part.
"""
import numpy as np

U = 2.0 ** -24

# K_EXP, counted from k_prep_img / k_prep_images, k_prep_aconst, k_scan_bias
# and the w fragments of k_scan_split / the z operand of k_scan_mfma.  The
# three kinds of term never share a pixel's share of S, so the count of one
# term is the largest of the three, plus the two bias adds:
#   A term  s (dx^2 + dy^2):        dx^2, dy^2 (one u between them: each
#           square's error is relative to its own square), the add, times s   3
#   B term  (s c c) (px^2 + py^2):  s c, times c; the squares (1), their add;
#           the product with b (exact inside the FP32 MFMA of k_scan_bias,
#           one rounding in k_scan_mfma's VALU form)                          5
#   X term  Re(w conj T), w = a conj(P), a = (-2 s c) d: s c (the -2 is
#           exact), times d: 2 u relative on each component of a; the two
#           products and the add of each component of w: 2 u of
#           |ar pr| + |ai pi|.  Both reach the term through
#           (|ar||pr| + |ai||pi|) |Tr| + (|ai||pr| + |ar||pi|) |Ti|
#           <= sqrt 2 |a||P||T|, so 4 sqrt 2 = 5.66 together; the
#           products with T are exact (FP32 MFMA, or exact bf16 pieces), the
#           add that pairs the re and im product is 1                  6.66 -> 7
#           (k_scan_mfma forms z = T P instead of w = a conj P: the same count)
#   bias    (A + B) and + X: one rounding each of a value <= S                2
K_EXP = 7 + 2

# K_DIR, counted from direct_dvp (scan_split.hip) and k_dvp_direct (scan.hip),
# with g = |d| + |c||T P| (s g^2 sums to S):
#   T P:   two products and an add per component, 2 u |T||P| each; times c
#          one more: 3 u |c||T P| per component, 3 sqrt 2 u |c||T P| in modulus
#   e = d - c T P: one rounding per component, u |e| <= u g in modulus
#          -> |delta e| <= (3 sqrt 2 + 1) u g, and |e|^2 moves by 2 |e| |delta e|
#          <= 2 (3 sqrt 2 + 1) u g^2                                    10.49
#   er^2 + ei^2 (one u between the squares, one for the add), times s       3
K_DIR = 14        # 13.49 rounded up

EPS = {0: 0.0, 1: 0.0, 2: 2.0 ** -16, 4: 2.0 ** -23}   # scan_split.hip's header
BAND = 1e-3       # relative half-width of the undetermined band at the guard ratio


def _blocks(nR, per_r, cap=1 << 21):
    step = max(1, cap // max(1, per_r))
    return [(r0, min(nR, r0 + step)) for r0 in range(0, nR, step)]


def dvp64(rotP, traP, dat, ctf, sig):
    """sum_i s |d - c (T P)|^2 in float64 from the FP32 operands -> [nImg, nR, nT]."""
    P, T = rotP.astype(np.complex128), traP.astype(np.complex128)
    d, c, s = dat.astype(np.complex128), ctf.astype(np.float64), sig.astype(np.float64)
    nImg, nR, nT = len(d), len(P), len(T)
    out = np.empty((nImg, nR, nT))
    for r0, r1 in _blocks(nR, nT * P.shape[1]):
        TP = T[None, :, :] * P[r0:r1, None, :]                      # [r, t, i]
        for l in range(nImg):
            e = d[l] - c[l] * TP
            out[l, r0:r1] = (e.real ** 2 + e.imag ** 2) @ s[l]
    return out


def sums(rotP, traP, dat, ctf, sig):
    """dict of [nImg, nR, nT] float64 arrays: the magnitude sums S_A, S_B, S_X,
    S = S_A + S_B + S_X, and G = |A| + |B| + |X| of the signed parts (the
    quantity the cancellation guard compares with |dvp|; G <= S), and
    AB = A + B, the value of a sample whose cross term is 0."""
    aP, aT = np.abs(rotP.astype(np.complex128)), np.abs(traP.astype(np.complex128))
    P, T = rotP.astype(np.complex128), traP.astype(np.complex128)
    d, c, s = dat.astype(np.complex128), ctf.astype(np.float64), sig.astype(np.float64)
    nImg, nR, nT = len(d), len(P), len(T)
    SA = (np.abs(s) * np.abs(d) ** 2).sum(1)
    A = (s * np.abs(d) ** 2).sum(1)
    SB, SX, B, X = (np.empty((nImg, nR, nT)) for _ in range(4))
    for r0, r1 in _blocks(nR, nT * P.shape[1]):
        aTP = aT[None, :, :] * aP[r0:r1, None, :]
        TP = T[None, :, :] * P[r0:r1, None, :]
        for l in range(nImg):
            SB[l, r0:r1] = (aTP ** 2) @ (np.abs(s[l]) * c[l] ** 2)
            SX[l, r0:r1] = aTP @ (2 * np.abs(s[l] * c[l]) * np.abs(d[l]))
            B[l, r0:r1] = (aP[r0:r1] ** 2 @ (s[l] * c[l] ** 2))[:, None]   # the kernels' |T| = 1
            X[l, r0:r1] = (TP * np.conj(d[l])).real @ (-2 * s[l] * c[l])
    SA3 = np.broadcast_to(SA[:, None, None], SB.shape)
    G = np.abs(A)[:, None, None] + np.abs(B) + np.abs(X)
    return dict(S_A=SA3, S_B=SB, S_X=SX, S=SA3 + SB + SX, G=G, AB=A[:, None, None] + B)


def budget_expanded(sm, nPxl, algo):
    return U * sm["S"] * (nPxl + K_EXP) + 2.0 ** -23 * sm["S_B"] + EPS[algo] * sm["S_X"]


def budget_direct(sm, nPxl):
    return U * sm["S"] * (nPxl + K_DIR)


def guard_form(sm, dvp, guard):
    """+1 where the guard certainly flags the sample (direct form), -1 where
    it certainly does not, 0 inside guard (1 +- BAND) where one rounding decides."""
    ratio = sm["G"] / np.maximum(np.abs(dvp), np.finfo(np.float64).tiny)
    return np.where(ratio > guard * (1 + BAND), 1, np.where(ratio < guard * (1 - BAND), -1, 0))


def budget(algo, guard, sm, dvp, nPxl):
    """Absolute error budget per sample [nImg, nR, nT].  algo 0 (and thx_dvp):
    the direct form.  algo 1: the expanded form (it has no guard).  algos 2, 4
    with guard > 0: the form the guard picks, the larger of the two inside the
    undetermined band."""
    if algo == 0:
        return budget_direct(sm, nPxl)
    be = budget_expanded(sm, nPxl, algo)
    if algo == 1 or not guard:
        return be
    bd = budget_direct(sm, nPxl)
    form = guard_form(sm, dvp, guard)
    return np.where(form > 0, bd, np.where(form < 0, be, np.maximum(be, bd)))


# ------------------------------------------------------------------ weights
def weights64(dvps, pR, pT, nK, order):
    """The class-merged marginals in float64.  dvps[k]: [nImg, nR, nT] of
    class k; order: the kIdx of the calls, in turn.  kIdx 0 starts afresh
    (every other class 0); the final baseline is the maximum over the classes
    scanned since.  -> wC [nImg, nK], wR [nImg, nK, nR], wT [nImg, nK, nT], base [nImg]."""
    live = {}
    for k in order:
        if k == 0:
            live = {}
        live[k] = dvps[k]
    nImg, nR, nT = next(iter(live.values())).shape
    base = np.max([d.max(axis=(1, 2)) for d in live.values()], axis=0)
    wC, wR, wT = np.zeros((nImg, nK)), np.zeros((nImg, nK, nR)), np.zeros((nImg, nK, nT))
    for k, d in live.items():
        e = np.exp(d - base[:, None, None])
        wR[:, k] = e @ pT
        wT[:, k] = np.einsum("lrt,r->lt", e, pR)
        wC[:, k] = wR[:, k] @ pR
    return wC, wR, wT, base


def weight_bounds(dvps, buds, pR, pT, nK, order, quantum=0.0):
    """Per-entry bounds (bC, bR, bT) of marginals computed by a kernel whose
    dvp may differ from dvps by the per-sample budget buds[k].  Each term e p
    moves by at most expm1(b_sample + b_top) of itself, b_top the largest
    budget of the image's samples (the kernel's baseline is its own maximum;
    over the classes scanned, as the baseline is); 1e-4 of the reference is
    added for the FP32 exponentials and sums (the bar of
    test_c3_product_scan_dvp_per_sample).  quantum: the absolute rounding of
    one rotation's term of wT where the kernel adds them in fixed point
    (k_scan_mfma: 2^-57 of a term scaled to its block maximum, <= 1), nR
    times per entry."""
    wC, wR, wT, base = weights64(dvps, pR, pT, nK, order)
    live = {}
    for k in order:
        if k == 0:
            live = {}
        live[k] = k
    btop = np.max([buds[k].max(axis=(1, 2)) for k in live], axis=0)
    bC, bR, bT = 1e-4 * wC, 1e-4 * wR, 1e-4 * wT
    nR = len(pR)
    for k in live:
        m = np.exp(dvps[k] - base[:, None, None]) * np.expm1(buds[k] + btop[:, None, None])
        bR[:, k] += m @ pT
        bT[:, k] += np.einsum("lrt,r->lt", m, pR) + nR * quantum
        bC[:, k] += (m @ pT) @ pR
    return bC, bR, bT


def merge_literal(dvps, pR, pT, nK, order):
    """The same result by a literal float64 loop over the calls that follows
    merge_baseline (scan_common.h) step by step: reset at kIdx 0, raise the
    baseline and rescale the other classes by exp(old - new) otherwise."""
    d0 = dvps[order[0]]
    nImg, nR, nT = d0.shape
    wC, wR, wT = np.full((nImg, nK), 7.0), np.full((nImg, nK, nR), 7.0), np.full((nImg, nK, nT), 7.0)
    base = np.full(nImg, np.nan)
    for kIdx in order:
        d = dvps[kIdx]
        for l in range(nImg):
            m, old = d[l].max(), base[l]
            if kIdx == 0:
                b = m
                for k in range(1, nK):
                    wC[l, k] = 0.0
                    wR[l, k, :] = 0.0
                    wT[l, k, :] = 0.0
            else:
                b = m if old != old else max(old, m)
                if b > old:
                    nf = np.exp(old - b)
                    for k in range(nK):
                        if k != kIdx:
                            wC[l, k] *= nf
                            wR[l, k, :] *= nf
                            wT[l, k, :] *= nf
            base[l] = b
            for r in range(nR):
                wR[l, kIdx, r] = sum(np.exp(d[l, r, t] - b) * pT[t] for t in range(nT))
            for t in range(nT):
                wT[l, kIdx, t] = sum(np.exp(d[l, r, t] - b) * pR[r] for r in range(nR))
            wC[l, kIdx] = sum(pR[r] * wR[l, kIdx, r] for r in range(nR))
    return wC, wR, wT, base


def worst(got, ref, bound):
    """Largest |got - ref| / bound; entries with bound 0 must match exactly
    (inf otherwise).  NaN in got counts as inf."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------- emulation
def bf16_round(x):
    """float32 -> the nearest bf16 (8 significant bits, ties to even), as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def split16(x):
    """(hi, lo) of scan_split.hip's split16: lo the bf16 of the exact residual."""
    x = np.asarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def split3(x):
    """(hi, mid, lo) with x = hi + mid + lo exactly."""
    x = np.asarray(x, np.float32)
    hi = bf16_round(x)
    r = x - hi
    mid = bf16_round(r)
    return hi, mid, bf16_round(r - mid)


# the products kept, as (piece of w, piece of T): three of four, six of nine
KEPT = {2: ((0, 0), (0, 1), (1, 0)),
        4: ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))}


def _f32(x):
    return np.asarray(x, np.float32)


def emu_parts32(rotP, traP, dat, ctf, sig):
    """The FP32 operands of the expanded form as the prep kernels form them:
    A [nImg], B [nImg, nR] (sequential FP32 sums), and w [nImg, nR, nPxl]
    (re, im) = a conj(P), a = (-2 s c) d."""
    d, c, s = dat, _f32(ctf), _f32(sig)
    dr, di = _f32(d.real), _f32(d.imag)
    pr, pi = _f32(rotP.real), _f32(rotP.imag)
    ta = s * (dr * dr + di * di)
    b = s * c * c
    p2 = pr * pr + pi * pi
    A = np.zeros(len(d), np.float32)
    B = np.zeros((len(d), len(pr)), np.float32)
    for i in range(d.shape[1]):
        A = A + ta[:, i]
        B = B + b[:, i, None] * p2[None, :, i]
    k = np.float32(-2.0) * s * c
    ar, ai = k * dr, k * di
    wr = ar[:, None, :] * pr[None] + ai[:, None, :] * pi[None]
    wi = ai[:, None, :] * pr[None] - ar[:, None, :] * pi[None]
    return A, B, wr, wi


def emu_expanded32(rotP, traP, dat, ctf, sig):
    """FP32 sequential sum of the expanded form with exact products (algo 1)."""
    A, B, wr, wi = emu_parts32(rotP, traP, dat, ctf, sig)
    tr, ti = traP.real.astype(np.float64), traP.imag.astype(np.float64)
    X = np.zeros(wr.shape[:2] + (len(tr),), np.float32)
    for i in range(wr.shape[2]):
        term = wr[:, :, None, i].astype(np.float64) * tr[None, None, :, i] + \
            wi[:, :, None, i].astype(np.float64) * ti[None, None, :, i]
        X = X + _f32(term)
    return (A[:, None] + B)[:, :, None] + X


def emu_x_split64(wr, wi, traP, algo, kept=None, planes=None):
    """The cross term from the split pieces, the kept products accumulated in
    float64.  kept: override of KEPT[algo]; planes: the T pieces that exist
    (a dropped plane reads as 0)."""
    sp = split16 if algo == 2 else split3
    W = [[p.astype(np.float64) for p in sp(wr)], [p.astype(np.float64) for p in sp(wi)]]
    T = [[p.astype(np.float64) for p in sp(_f32(traP.real))],
         [p.astype(np.float64) for p in sp(_f32(traP.imag))]]
    X = 0.0
    for (iw, it) in (KEPT[algo] if kept is None else kept):
        if planes is not None and it not in planes:
            continue
        X = X + np.einsum("lri,ti->lrt", W[0][iw], T[0][it]) + np.einsum("lri,ti->lrt", W[1][iw], T[1][it])
    return X


def emu_x_exact64(wr, wi, traP):
    return np.einsum("lri,ti->lrt", wr.astype(np.float64), traP.real.astype(np.float64)) + \
        np.einsum("lri,ti->lrt", wi.astype(np.float64), traP.imag.astype(np.float64))


def emu_split(rotP, traP, dat, ctf, sig, algo, kept=None, planes=None):
    """A + B in FP32 plus the split cross term in float64 (the split's own
    loss, without the accumulation rounding)."""
    A, B, wr, wi = emu_parts32(rotP, traP, dat, ctf, sig)
    AB = (A[:, None] + B).astype(np.float64)
    return AB[:, :, None] + emu_x_split64(wr, wi, traP, algo, kept, planes)


def emu_direct32(rotP, traP, dat, ctf, sig):
    """FP32 sequential sum of the direct form, operation by operation as
    direct_dvp writes it (no contraction)."""
    pr, pi = _f32(rotP.real)[None, :, None], _f32(rotP.imag)[None, :, None]
    tr, ti = _f32(traP.real)[None, None], _f32(traP.imag)[None, None]
    dr, di = _f32(dat.real)[:, None, None], _f32(dat.imag)[:, None, None]
    c, s = _f32(ctf)[:, None, None], _f32(sig)[:, None, None]
    acc = np.zeros((dat.shape[0], rotP.shape[0], traP.shape[0]), np.float32)
    for i in range(dat.shape[1]):
        qr = tr[..., i] * pr[..., i] - ti[..., i] * pi[..., i]
        qi = tr[..., i] * pi[..., i] + ti[..., i] * pr[..., i]
        er = dr[..., i] - c[..., i] * qr
        ei = di[..., i] - c[..., i] * qi
        acc = acc + (er * er + ei * ei) * s[..., i]
    return acc
