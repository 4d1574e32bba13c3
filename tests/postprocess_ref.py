"""numpy restatement of Postprocess::run (src/Postprocess.cpp:50-183) after its
"true FSC" (tests/fsc_masked_ref.py): resP at 0.143, mergeAB (:207-213),
fscWeightingFilter (src/Functions/Filter.cpp:144-167), bFactorEst
(src/Functions/Spectrum.cpp:414-453) with GSL's unweighted fit_linear in closed
form, sharpen (:402-412: bFactorFilter, Filter.cpp:29-44, then lowPassFilter,
:69-92), irfftn and softMask with bg = 0; written independently of
csrc/postprocess.hip.  ``dtype`` is the working precision of the maps and of
the filters' factors (np.float64: the reference the tests compare against;
np.float32: the same code, for the float32 error e32); shell sums and the fit
are float64 either way.  A plain module: import it from a test.
"""
import types

import numpy as np

import fsc_masked_ref

B_FACTOR_EST_LOW_RES = 10.0
EDGE_WIDTH_FT = 4.0


def _grid(N):
    ax = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)
    return np.meshgrid(ax, ax, np.arange(N // 2 + 1), indexing="ij")    # k, j, i


def shell_index(N):
    """AROUND(NORM_3(i, j, k)) from the integer i^2 + j^2 + k^2 (bFactorEst's form)"""
    return fsc_masked_ref.shell_index(N)


def shell_index_fp32(N):
    """fscWeightingFilter's literal expression in RFLOAT = float:
    AROUND(NORM_3(i / N, j / N, k / N) * N)"""
    k, j, i = _grid(N)
    n = np.float32(N)
    x, y, z = (v.astype(np.float32) / n for v in (i, j, k))
    f = np.sqrt(x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2
                + z.astype(np.float64) ** 2).astype(np.float32)     # gsl_hypot3, into an RFLOAT
    return np.rint(f * n).astype(np.int64)


def freq2(N, dtype):
    """(i/N)^2 + (j/N)^2 + (k/N)^2 in ``dtype``"""
    k, j, i = _grid(N)
    n = dtype(N)
    x, y, z = (v.astype(dtype) / n for v in (i, j, k))
    return (x * x + y * y + z * z).astype(dtype)


def res_p(f, thres, rL=1):
    return fsc_masked_ref.res_p(f, thres, rL)


def r_low(N, pixel_size, low_res=B_FACTOR_EST_LOW_RES):
    """AROUND(resA2P(1 / lowRes, N, pixelSize)) in RFLOAT"""
    return int(np.rint(np.float32(N) * np.float32(pixel_size) / np.float32(low_res)))


def merge(A, B):
    return (A + B) / 2


def fsc_weight(fsc, dtype=np.float64):
    """sqrt(max(0, 2 fsc / (1 + fsc))) per shell, as an RFLOAT of ``dtype``"""
    f = np.asarray(fsc, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.fmax(0.0, 2 * f / (1 + f))).astype(dtype)


def fsc_weighting(F, fsc, u=None, dtype=np.float64, weight=fsc_weight):
    """fscWeightingFilter: times the shell's weight, exactly 0 from len(fsc) on"""
    if u is None:
        u = shell_index(F.shape[0])
    w = np.concatenate([weight(fsc, dtype), np.zeros(1, dtype)])
    return F * w[np.minimum(u, len(fsc))]


def fit_linear(x, y):
    """gsl_fit_linear, unweighted: c1 = sum (x - mx)(y - my) / sum (x - mx)^2"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx = x - x.mean()
    c1 = float((dx * (y - y.mean())).sum() / (dx * dx).sum())
    return float(y.mean() - c1 * x.mean()), c1


def b_factor_est(F, rU, rL, u=None, inclusive=False):
    """bFactorEst over the shells [rL, rU): returns (bFactor, c0, x, y, status);
    status 1 (and bFactor 0) where the reference's fit is undefined"""
    N = F.shape[0]
    if u is None:
        u = shell_index(N)
    hi = rU + 1 if inclusive else rU
    n = hi - rL
    if n < 2:
        return 0.0, 0.0, np.zeros(0), np.zeros(0), 1
    m = (u >= rL) & (u < hi)
    s = np.bincount(u[m] - rL, weights=np.abs(F[m]).astype(np.float64), minlength=n)
    c = np.bincount(u[m] - rL, minlength=n)
    if np.any(c == 0) or np.any(~(s > 0)):
        return 0.0, 0.0, np.zeros(0), np.zeros(0), 1
    x = ((np.arange(rL, hi).astype(np.float32) / np.float32(N)) ** 2).astype(np.float64)
    y = np.log(s / c)
    c0, c1 = fit_linear(x, y)
    return 2 * c1, c0, x, y, 0


def b_factor_filter(F, b, dtype=np.float64, expo=-0.5):
    """bFactorFilter: times exp(-0.5 b f^2)"""
    if b == 0:
        return F
    return F * np.exp(dtype(expo) * dtype(b) * freq2(F.shape[0], dtype)).astype(dtype)


def low_pass_factor(f, thres, ew, dtype=np.float64):
    """lowPassFilter's factor at the norm f: 1 for f < thres, 0 for f > thres +
    ew, cos((f - thres) pi / ew) / 2 + 0.5 between (comparisons as written)"""
    f, thres, ew = np.asarray(f, dtype), dtype(thres), dtype(ew)
    mid = (np.cos((f - thres) * dtype(np.pi) / ew) / dtype(2) + dtype(0.5)).astype(dtype)
    return np.where(f < thres, dtype(1), np.where(f > thres + ew, dtype(0), mid)).astype(dtype)


def low_pass(F, thres, ew, dtype=np.float64):
    if not (ew > 0 and thres >= 0):
        return F
    return F * low_pass_factor(np.sqrt(freq2(F.shape[0], dtype)), thres, ew, dtype)


def sharpen(F, thres, ew, b, dtype=np.float64, expo=-0.5):
    return low_pass(b_factor_filter(F, b, dtype, expo), thres, ew, dtype)


def to_real(F, N):
    """FFT::bw with its 1 / N^3 (numpy's irfftn normalises)"""
    return np.fft.irfftn(F, s=(N, N, N), axes=(0, 1, 2))


def postprocess(A, B, alpha, pixel_size, seed=0, b_factor=None, low_res=B_FACTOR_EST_LOW_RES,
                edge_ft=EDGE_WIDTH_FT, dtype=np.float64, mutate=None):
    """The whole chain.  ``mutate`` names one deliberate mistake, for the tests
    that show the GPU bound sees it: "exponent" (-0.25 for -0.5), "inclusive"
    (the fit over [rL, res]), "edge" (ew = edge_ft / (2N)), "no_sqrt" (the FSC
    weight without its square root)."""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    N = A.shape[0]
    n_shell = N // 2 - 1
    o = fsc_masked_ref.masked_fsc(A, B, n_shell, alpha, seed, dtype)
    A, B = np.asarray(A).astype(ctype), np.asarray(B).astype(ctype)
    alpha = np.asarray(alpha).astype(dtype)
    u = shell_index(N)
    o.res = res_p(o.fsc, 0.143)
    o.r_low = r_low(N, pixel_size, low_res)
    merged = merge(A, B).astype(ctype)
    o.average = to_real(merged, N).astype(dtype)
    weight = fsc_weight
    if mutate == "no_sqrt":
        def weight(f, dt):
            return (fsc_weight(f, np.float64) ** 2).astype(dt)
    weighted = fsc_weighting(merged, o.fsc, u, dtype, weight).astype(ctype)
    if b_factor is None:
        o.b_factor, o.c0, o.x, o.y, o.status = b_factor_est(weighted, o.res, o.r_low, u,
                                                            inclusive=mutate == "inclusive")
    else:
        o.b_factor, o.c0, o.x, o.y, o.status = float(b_factor), 0.0, np.zeros(0), np.zeros(0), 0
    o.n_fit = max(0, o.res - o.r_low) if b_factor is None else 0
    ew = dtype(edge_ft) / dtype(2 * N if mutate == "edge" else N)
    ft = sharpen(weighted, dtype(o.res) / dtype(N), ew, dtype(o.b_factor), dtype,
                 -0.25 if mutate == "exponent" else -0.5).astype(ctype)
    one = dtype(1)
    o.sharp = (to_real(ft, N).astype(dtype) * (one - (one - alpha))).astype(dtype)
    o.resolution_A = N * pixel_size / o.res if o.res > 0 else np.inf
    return o
