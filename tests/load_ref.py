"""numpy float64 restatement of thx_pf_load (thunder_amd/csrc/load.hip), written
from Particle::load (src/Particle.cpp:401-556; sampleACG, src/Geometry/
DirectionalStat.cpp:39-91; quaternion_mul, src/Geometry/Euler.cpp:13-26) and
the draw layout of the kernel's header comment, on the counter RNG of
philox_ref.  A plain module: import it from a test.

Image l owns 8 lanes; lane j owns the stream (l, stream_id, j) and the
particles i = j (mod 8) of every set, in rising order.  With n_j = (n + 7 - j)
// 8 the lane's share of a set of n, its counter runs over 4 nR_j rotation
uniforms (pf_ref.rotation_draws, unchanged), then 2 nT_j translation uniforms,
then 2 nD_j defocus uniforms (the cosine branch kept), then nR_j sign uniforms.
"""
from collections import namedtuple

import numpy as np

import pf_ref
import philox_ref
from oracle import particle as op

GROUP = pf_ref.GROUP

# pert [n, mR, 4] sampleACG's draws, sign [n, mR] the +-1 of the base rotation,
# quat = pert (sign q); the priors pT / pD; d, pD empty [n, 0] with mD = 0
Loaded = namedtuple("Loaded", "quat trans d pT pD pert sign")


def _share(n, lane):
    """How many of a set's n particles lane `lane` owns."""
    return (np.uint64(n + GROUP - 1) - lane) // np.uint64(GROUP)


def _lanes(n_img, m):
    """(image, lane, turn) of the particles 0 .. m-1 of every image, flat."""
    l = np.repeat(np.arange(n_img, dtype=np.uint64), m)
    i = np.tile(np.arange(m, dtype=np.uint64), n_img)
    return l, i % np.uint64(GROUP), i // np.uint64(GROUP)


def load(top_quat, k, top_trans, sd, top_d, sd_d, mR, mT, mD, seed, stream_id):
    """thx_pf_load without the rotation statistics (pR and vari[0..2] pass
    through inferACG's fixed point: oracle.particle.balance_rot / cal_vari_rot
    on a cloud give them, see stats)."""
    top_quat, k, top_trans, sd = (np.asarray(x, np.float64) for x in (top_quat, k, top_trans, sd))
    n = len(top_quat)
    two, four = np.uint64(2), np.uint64(4)

    # ---- rotations (:462-489): pert ~ sampleACG(k1, k2, k3), uncapped;
    # part = quaternion_mul(pert, +-q), + where gsl_ran_flat(-1, 1) >= 0
    pert = pf_ref.rotation_draws(n, mR, np.sqrt(k), seed, stream_id)
    l, lane, turn = _lanes(n, mR)
    base = four * _share(mR, lane) + two * _share(mT, lane) + two * _share(mD, lane)
    u = philox_ref.uniform(seed, l, stream_id, lane, base + turn)
    sign = np.where(-1.0 + 2.0 * u >= 0.0, 1.0, -1.0).reshape(n, mR)
    quat = np.empty((n, mR, 4))
    for a in range(n):
        quat[a] = op.qmul(pert[a], sign[a][:, None] * top_quat[a][None, :])

    # ---- translations (:509-530): gsl_ran_bivariate_gaussian(s0, s1, rho 0) + t
    l, lane, turn = _lanes(n, mT)
    gx, gy = philox_ref.gauss2(seed, l, stream_id, lane, four * _share(mR, lane) + two * turn)
    il = l.astype(int)
    trans = np.stack([top_trans[il, 0] + gx * sd[il, 0], top_trans[il, 1] + gy * sd[il, 1]],
                     axis=1).reshape(n, mT, 2)
    pT = np.array([pf_ref.balance_trans(trans[a]) for a in range(n)])

    # ---- defocus factors (:539-551): d + gsl_ran_gaussian(s)
    d, pD = np.empty((n, 0)), np.empty((n, 0))
    if mD > 0:
        top_d, sd_d = np.asarray(top_d, np.float64), np.asarray(sd_d, np.float64)
        l, lane, turn = _lanes(n, mD)
        g, _ = philox_ref.gauss2(seed, l, stream_id, lane,
                                 four * _share(mR, lane) + two * _share(mT, lane) + two * turn)
        il = l.astype(int)
        d = (top_d[il] + g * sd_d[il]).reshape(n, mD)
        pD = np.array([op.balance_defocus(d[a]) for a in range(n)])
    return Loaded(quat, trans, d, pT, pD, pert, sign)


def stats(quat, trans, d):
    """(pR [mR], vari [6]) of one image's clouds: balanceWeight(PAR_R) and
    calVari(PAR_R / PAR_T / PAR_D) (:495-499, :530, :551), sD = 0 without
    defocus samples."""
    k = op.cal_vari_rot(quat)
    s = op.cal_vari_trans(trans) if len(trans) > 1 else (0.0, 0.0)
    sD = op.cal_vari_defocus(d) if len(d) else 0.0
    return op.balance_rot(quat), np.array([k[0], k[1], k[2], s[0], s[1], sD])
