"""Between two rounds: what Optimiser::run does with the top particles
(Particle::rank1st, ``Expectation.rank1st()``) after the expectation
(src/Optimiser.cpp:3691-3833), over csrc/round.hip.

    refreshClassDistr      (:3691)       class_distribution(cls, nK, group)
    refreshVariance        (:3732)       refresh_variance(vari, two_d, group)
    refreshRotationChange  (:3767)       rank1st_change(r1, prev) -> diffR,
                                         refresh_rotation_change(diffR, group)
    reCentreImg, reMaskImg (:3804-3833)  recentre(..., remask=(rMask, edge))

The per-image terms are device kernels; the robust statistics over all
particles (stat_MAS, src/Functions/Functions.cpp:254-275) are one sort of a
vector of nPar numbers after the gather over the ``torch.distributed`` group,
like normCorrection's median.
"""
import torch

from . import ingest
from ._lib import check, lib
from .ops import _ptr, _req, _stream


def rank1st_change(r1, prev):
    """thx_rank1st_diff.  r1 = (cls, quat, trans, d) -- the first four of
    Expectation.rank1st(), any of them None -- and prev the same tuple from
    the last round, updated in place to r1.  Returns (diffR, diffT, diffD,
    sameC), None where the group is absent: 1 - |<q', q>|, |t' - t|,
    |d' - d| and sameC = 1 where the class is unchanged (the equality
    Particle::diffTopC returns despite its name)."""
    cls, quat, trans, d = r1[:4]
    pcls, pquat, ptrans, pd = prev[:4]
    n = next(t.shape[0] for t in (quat, trans, d, cls) if t is not None)
    dev = next(t.device for t in (quat, trans, d, cls) if t is not None)

    def group(cur, prv, shape, dtype, name):
        if cur is None:
            return None, None, None
        _req(cur, dtype, shape, name)
        _req(prv, dtype, shape, "prev " + name)
        return cur, prv, torch.empty(n, dtype=dtype, device=dev)

    q, pq, dR = group(quat, pquat, (n, 4), torch.float64, "quat")
    t, pt, dT = group(trans, ptrans, (n, 2), torch.float64, "trans")
    dd, pdd, dD = group(d, pd, (n,), torch.float64, "d")
    c, pc, sC = group(cls, pcls, (n,), torch.int32, "cls")
    check(lib().thx_rank1st_diff(n, _ptr(q), _ptr(pq), _ptr(dR), _ptr(t), _ptr(pt), _ptr(dT),
                                 _ptr(dd), _ptr(pdd), _ptr(dD), _ptr(c), _ptr(pc), _ptr(sC),
                                 _stream(dev)), "thx_rank1st_diff")
    return dR, dT, dD, sC


def recentre(oriFT, imgFT, r1_trans, offS, trans=None, prev_trans=None, remask=None):
    """thx_recentre (Optimiser::reCentreImg), in place: with t = r1_trans[l],
    offS[l] -= t, imgFT[l] = oriFT[l] shifted by the updated offS[l], the
    cloud trans [n, mLT, 2] -= t, prev_trans [n, 2] -= t and r1_trans -> 0.
    imgFT (None: the state only) is [n, N, N/2+1] complex64 like oriFT.
    remask = (rMask, edge): reMaskImg on the shifted images (thx_remask)."""
    n = r1_trans.shape[0]
    _req(r1_trans, torch.float64, (n, 2), "r1_trans")
    _req(offS, torch.float64, (n, 2), "offS")
    N, mLT = 0, 0
    if imgFT is not None:
        N = imgFT.shape[1]
        _req(imgFT, torch.complex64, (n, N, N // 2 + 1), "imgFT")
        _req(oriFT, torch.complex64, (n, N, N // 2 + 1), "oriFT")
    if trans is not None:
        mLT = trans.shape[1]
        _req(trans, torch.float64, (n, mLT, 2), "trans")
    if prev_trans is not None:
        _req(prev_trans, torch.float64, (n, 2), "prev_trans")
    check(lib().thx_recentre(n, N, _ptr(oriFT) if imgFT is not None else None, _ptr(imgFT),
                             _ptr(r1_trans), _ptr(offS), mLT, _ptr(trans), _ptr(prev_trans),
                             _stream(r1_trans.device)), "thx_recentre")
    if remask is not None and imgFT is not None and n:
        ingest.remask(imgFT, *remask)
    return imgFT


def _all_reduce(t, group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def _all_gather(x, group):
    """The values of every rank of the group, concatenated (ranks may hold
    different numbers of images)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return x
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, x.detach().cpu(), group=group)
    return torch.cat(parts)


def class_count(cls, nK, count=None):
    """thx_class_count: count [nK] float64 (made, zeroed, when None) +=
    the number of images of each class; classes outside [0, nK) are left out."""
    n = cls.shape[0]
    _req(cls, torch.int32, (n,), "cls")
    if count is None:
        count = torch.zeros(nK, dtype=torch.float64, device=cls.device)
    _req(count, torch.float64, (nK,), "count")
    check(lib().thx_class_count(n, _ptr(cls), nK, _ptr(count), _stream(cls.device)),
          "thx_class_count")
    return count


def class_distribution(cls, nK, group=None):
    """refreshClassDistr: the share of every class among the images of all
    ranks of `group` [nK] float64 (after resample(K, PAR_C) the reference's k
    draws per image all give the image's class, so its normalised tally is
    this histogram).  Raises ValueError when no image of any rank has a class
    in [0, nK): there is no distribution to normalise."""
    count = _all_reduce(class_count(cls, nK), group)
    total = count.sum()
    if float(total) == 0.0:
        raise ValueError("class_distribution: no image with a class in [0, nK)")
    return count / total


def stat_mas(x):
    """stat_MAS: (median, 1.4826 x the median absolute deviation from it),
    medians by gsl_stats_quantile_from_sorted_data(..., 0.5): with
    h = (n - 1) / 2, (1 - frac h) x[floor h] + frac h x[floor h + 1]."""
    x = torch.as_tensor(x, dtype=torch.float64).reshape(-1)
    if x.numel() == 0:
        raise ValueError("stat_mas of an empty set")

    def median(v):
        v = torch.sort(v).values
        n = v.numel()
        lhs = (n - 1) // 2
        delta = (n - 1) / 2 - lhs
        if lhs == n - 1:
            return v[lhs]
        return (1 - delta) * v[lhs] + delta * v[lhs + 1]

    m = median(x)
    return float(m), float(median((x - m).abs()) * 1.4826)


def refresh_variance(vari, two_d, group=None):
    """refreshVariance: stat_mas over all particles of rVari = (k1 k2 k3)^(1/6)
    (2D: k1), s0 and s1 from Expectation.rank1st()'s vari [n, 6].  Returns
    {"rVari": (median, std), "tVariS0": ..., "tVariS1": ...}."""
    v = _all_gather(vari, group)
    r = v[:, 0] if two_d else (v[:, 0] * v[:, 1] * v[:, 2]) ** (1.0 / 6)
    return {"rVari": stat_mas(r), "tVariS0": stat_mas(v[:, 3]), "tVariS1": stat_mas(v[:, 4])}


def refresh_rotation_change(diffR, group=None):
    """refreshRotationChange: stat_mas of the images' diffR
    (rank1st_change) over all particles -> (rChange, stdRChange)."""
    return stat_mas(_all_gather(diffR, group))
