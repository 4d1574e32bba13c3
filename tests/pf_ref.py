"""numpy float64 restatement of the kernels that turn one particle-filter
phase of the 3D driver into the next (thunder_amd/csrc/optimiser.hip), written
from the reference's lines and the kernels' header comments, on the counter
RNG of philox_ref.  A plain module: import it from a test.

  perturb3d      Particle::perturb(PAR_R / PAR_T) + reCentre + balanceWeight(PAR_T)
                 (src/Particle.cpp:1149-1289, 2342-2372, 2473-2495; sampleACG,
                 src/Geometry/DirectionalStat.cpp:39-91)
  class_draw     the class draw of the K > 1 reseed (src/Optimiser.cpp:1933-1965;
                 resample(PAR_C) / shuffle(PAR_C) / rand(cls), src/Particle.cpp:
                 1296-1340, 2206-2230, 2109-2118)
  converge_step  the stopping rule (src/Optimiser.cpp:1510-1615,
                 OPTIMISER_COMPRESS_CRITERIA; variR / variT / variD,
                 src/Particle.cpp:611-645)
  compact        the list of images still running

Where the kernels' draws are laid out (which the reference, on one gsl engine
per thread, does not fix): image l owns 8 lanes; lane j owns the stream
(l, stream_id, j) and the particles i = j (mod 8) in rising order, first all
its rotations (four uniforms each), then its translations (two uniforms each,
two more for a re-drawn one).
"""
from collections import namedtuple

import numpy as np

import philox_ref
from oracle import particle as op
from oracle import symmetry as osym

GROUP = 8                         # lanes per image
PERTURB_K_MAX = op.PERTURB_K_MAX
PEAK_FACTOR_C = 1.0 - 1e-2        # PARTICLE_PEAK_FACTOR_C, include/Particle.h:55
DECREASE_FACTOR = 0.95            # PARTICLE_FILTER_DECREASE_FACTOR
SD_FLOOR, PDF_FLOOR = 1e-6, 1e-300   # the kernel's floors in balanceWeight(PAR_T)
CLASS_SHUFFLE, CLASS_DRAW = 0x5F1E, 0x5E5A   # counter word c of k_pf_class's two streams
DBL_MAX = np.finfo(np.float64).max

Perturbed = namedtuple("Perturbed", "quat trans pT guard_t guard_sym redrawn")


def balance_trans(t, floors=True):
    """balanceWeight(PAR_T) (src/Particle.cpp:2342-2372, rho = 0) of one set
    t [mT, 2]: 1 / N2(t - m; s0, s1, 0) with the sample mean and gsl_stats_sd_m,
    normalised to sum 1.  floors: the kernel's departures -- sd >= 1e-6, sd = 1
    for a single particle (gsl's n - 1 = 0), pdf >= 1e-300."""
    t = np.asarray(t, np.float64)
    m = t.mean(axis=0)
    if len(t) > 1:
        s = np.sqrt(np.sum((t - m) ** 2, axis=0) / (len(t) - 1))
    else:
        s = np.ones(2)
    if floors:
        s = np.maximum(SD_FLOOR, s)
    z = (t - m) / s
    p = np.exp(-(z[:, 0] ** 2 + z[:, 1] ** 2) / 2) / (2 * np.pi * s[0] * s[1])
    if floors:
        p = np.maximum(p, PDF_FLOOR)
    w = 1.0 / p
    return w / w.sum()


def rotation_draws(n_img, mR, sdv, seed, stream_id):
    """sampleACG's draws d [n_img, mR, 4]: N(0, diag(1, sdv^2)) normalised, sdv
    [n_img, 3] the standard deviations.  Particle i is draw i // 8 of lane
    i % 8: counters 4 (i // 8) .. + 3, two Box-Muller pairs, cosine then sine."""
    l = np.repeat(np.arange(n_img, dtype=np.uint64), mR)
    i = np.tile(np.arange(mR, dtype=np.uint64), n_img)
    lane, w = i % np.uint64(GROUP), np.uint64(4) * (i // np.uint64(GROUP))
    a0, a1 = philox_ref.gauss2(seed, l, stream_id, lane, w)
    a2, a3 = philox_ref.gauss2(seed, l, stream_id, lane, w + np.uint64(2))
    sdv = np.repeat(np.asarray(sdv, np.float64), mR, axis=0)
    d = np.stack([a0, a1 * sdv[:, 0], a2 * sdv[:, 1], a3 * sdv[:, 2]], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.reshape(n_img, mR, 4)


def _counterpart_gap(q, quats, anchor):
    """|<copy, anchor>| of q and of every conj(s) q, best minus second best."""
    s = [abs(float(np.dot(q, anchor)))]
    for sq in quats:
        s.append(abs(float(np.dot(osym.quat_mul(sq * np.array([1.0, -1, -1, -1]), q), anchor))))
    s = np.sort(s)
    return s[-1] - s[-2]


def perturb3d(quat, trans, mean, k, sd, pf, transS, transM, seed, stream_id, sym=None):
    """One k_pf_perturb launch without a done mask on clouds quat [nImg, mR, 4],
    trans [nImg, mT, 2] about mean [nImg, 4] with k [nImg, 3], sd [nImg, 2]; sym:
    the non-identity symmetry elements [n, 4] or None.

    Returns Perturbed(quat, trans, pT, guard_t, guard_sym, redrawn):
      guard_t [nImg]    min over particles of | |t + step| - transM |: how close
                        the re-draw decision came to a tie;
      guard_sym [nImg]  min over particles of the gap between the best and the
                        second-best |<copy, mean>| over symmetry copies (inf
                        without symmetry);
      redrawn [nImg, mT] bool."""
    quat, trans = np.asarray(quat, np.float64), np.asarray(trans, np.float64)
    mean, k, sd = (np.asarray(x, np.float64) for x in (mean, k, sd))
    nImg, mR = quat.shape[:2]
    mT = trans.shape[1]

    # ---- rotations: r <- mean d conj(mean) r (src/Particle.cpp:1206-1232)
    sdv = pf * np.sqrt(np.minimum(PERTURB_K_MAX, k))
    d = rotation_draws(nImg, mR, sdv, seed, stream_id)
    Q = np.empty_like(quat)
    guard_sym = np.full(nImg, np.inf)
    for l in range(nImg):
        m = np.tile(mean[l], (mR, 1))
        r = op.qmul(m, op.qmul(d[l], op.qmul(op.conj(m), quat[l])))
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        if sym is not None and len(sym):
            guard_sym[l] = min(_counterpart_gap(q, sym, mean[l]) for q in r)
            r = osym.symmetrise(r, sym, anchor=mean[l])      # symmetrise(&mean), :1234
        Q[l] = r

    # ---- translations (:1247-1272) and reCentre (:2473-2495); lane j has
    # drawn 4 per rotation it owns when its translations start
    T = trans.copy()
    redrawn = np.zeros((nImg, mT), bool)
    dist = np.zeros((nImg, mT))
    li = np.repeat(np.arange(nImg, dtype=np.uint64), GROUP)
    ln = np.tile(np.arange(GROUP, dtype=np.uint64), nImg)
    ctr = np.uint64(4) * ((np.uint64(mR + GROUP - 1) - ln) // np.uint64(GROUP))
    il, jl = li.astype(int), ln.astype(int)
    for n in range((mT + GROUP - 1) // GROUP):
        i = n * GROUP + jl
        on = i < mT
        gx, gy = philox_ref.gauss2(seed, li, stream_id, ln, ctr)
        ctr = ctr + np.where(on, np.uint64(2), np.uint64(0))
        a, b, lo = il[on], i[on], np.flatnonzero(on)
        x = T[a, b, 0] + gx[on] * sd[a, 0] * pf
        y = T[a, b, 1] + gy[on] * sd[a, 1] * pf
        dist[a, b] = np.sqrt(x * x + y * y)
        far = dist[a, b] > transM
        hx, hy = philox_ref.gauss2(seed, li, stream_id, ln, ctr)
        x = np.where(far, hx[on] * transS, x)
        y = np.where(far, hy[on] * transS, y)
        ctr[lo[far]] += np.uint64(2)
        T[a, b, 0], T[a, b, 1] = x, y
        redrawn[a, b] = far
    guard_t = np.abs(dist - transM).min(axis=1)
    pT = np.array([balance_trans(T[l]) for l in range(nImg)])
    return Perturbed(Q, T, pT, guard_t, guard_sym, redrawn)


def class_draw(wC, seed, stream_id):
    """k_pf_class on marginals wC [nImg, K] float32: cls [nImg].

    keepHalfHeightPeak(PAR_C) with PEAK_FACTOR_C, then resample(K, PAR_C) and
    rand(cls): of the K systematic draws u0 + j / K only the one rand picks, j
    uniform on 0 .. K-1, is carried out.  Position i of the shuffled set holds
    class pm[i], pm the identity after gsl_ran_shuffle's swaps (i = K-1 .. 1,
    j uniform on 0 .. i) with the integer draws (x (i + 1)) >> 32 of the stream
    (l, stream_id, CLASS_SHUFFLE).  The weights are the reset prior 1 / K times
    the cut marginal, the cdf is left unnormalised and the draw scaled by its
    total instead: the arithmetic below, IEEE double throughout.  u0 and j are
    draws 0 and 1 of the stream (l, stream_id, CLASS_DRAW)."""
    wC = np.asarray(wC, np.float32)
    nImg, K = wC.shape
    l = np.arange(nImg, dtype=np.uint64)
    pm = np.tile(np.arange(K), (nImg, 1))
    rows = np.arange(nImg)
    for step, i in enumerate(range(K - 1, 0, -1)):
        x = philox_ref.word0(seed, l, stream_id, CLASS_SHUFFLE, step)
        j = ((x * np.uint64(i + 1)) >> np.uint64(32)).astype(int)
        pi, pj = pm[rows, i].copy(), pm[rows, j].copy()
        pm[rows, i], pm[rows, j] = pj, pi
    mx = np.maximum(np.float32(0), wC.max(axis=1)).astype(np.float64)
    hh = mx * PEAK_FACTOR_C
    v = np.take_along_axis(wC, pm, axis=1).astype(np.float64)
    cut = np.where(v < hh[:, None], 0.0, v - hh[:, None]) / K
    cdf = np.zeros((nImg, K))
    acc = np.zeros(nImg)
    for i in range(K):                   # the running sum in index order
        acc = acc + cut[:, i]
        cdf[:, i] = acc
    u0 = philox_ref.uniform(seed, l, stream_id, CLASS_DRAW, 0) / K
    j = ((philox_ref.word0(seed, l, stream_id, CLASS_DRAW, 1) * np.uint64(K)) >> np.uint64(32))
    uj = (u0 + j.astype(np.float64) * 1.0 / K) * cdf[:, -1]
    # while (uj > cdf[i]) i++, ending at the last entry
    first = np.argmax(~(uj[:, None] > cdf), axis=1)
    first = np.where(np.any(~(uj[:, None] > cdf), axis=1), first, K - 1)
    return pm[rows, first].astype(np.int32)


def converge_state(n_img, with_d=False):
    """The stopping rule's state before the first phase: no image done, the
    bests at DBL_MAX (src/Optimiser.cpp: variR = variT = variD = DBL_MAX)."""
    st = {"done": np.zeros(n_img, np.int32), "nP": np.zeros(n_img, np.int32),
          "bestR": np.full(n_img, DBL_MAX), "bestT": np.full(n_img, DBL_MAX)}
    if with_d:
        st["bestD"] = np.full(n_img, DBL_MAX)
    return st


def converge_step(st, phase, min_phase, last_phase, k, sd, sdD=None, two_d=False):
    """One phase of src/Optimiser.cpp:1510-1615 on the state st (modified and
    returned): for images still running, from min_phase on, there is room when
    variR, variT (or variD, with sdD) fell strictly below 0.95 of the smallest
    value so far; the bests then take the minimum; N_PHASE_WITH_NO_VARI_DECREASE
    = 1 phase without room ends the image with nP = phase, and so does
    last_phase (the loop's end).  The bests count from min_phase: whatever they
    held before is DBL_MAX to the first check, which therefore finds room."""
    k, sd = np.asarray(k, np.float64), np.asarray(sd, np.float64)
    for l in range(len(st["done"])):
        if st["done"][l]:
            continue
        stop = phase >= last_phase
        if phase >= min_phase:
            cur = {"bestR": k[l, 0] if two_d else (k[l, 0] * k[l, 1] * k[l, 2]) ** (1.0 / 6),
                   "bestT": sd[l, 0] * sd[l, 1]}
            if sdD is not None:
                cur["bestD"] = float(sdD[l])
            if phase == min_phase:
                for name in cur:
                    st[name][l] = DBL_MAX
            room = any(v < st[name][l] * DECREASE_FACTOR for name, v in cur.items())
            for name, v in cur.items():
                if v < st[name][l]:
                    st[name][l] = v
            stop = stop or not room
        if stop:
            st["done"][l] = 1
            st["nP"][l] = phase
    return st


def converge_script():
    """Twelve phases (min_phase 2, last_phase 11) of scripted spreads for ten
    images, and the phase each ends at, read off src/Optimiser.cpp:1510-1615
    by hand.  Returns (k [12, 10, 3], sd [12, 10, 2], sdD [12, 10], nP without
    the defocus criterion, nP with it); both nP hold in 3D and in 2D.

    k = (r^2, r^2, r^2), so variR = r in 3D and r^2 in 2D, except where noted.
      0  all constant: room at 2 (the first check), none at 3 -> 3; from phase
         8 on its spreads collapse, which a finished image must not notice
      1  r falls 10 % a phase up to phase 6, then stays -> 7
      2  only s0 falls, 10 % a phase up to phase 5 -> 6
      3  variT exactly 1 at phase 2 and exactly 0.95 at phase 3 (s0 = 0.95, s1
         = 1; 1 * 0.95 == 0.95), k = (64, 1, 1) with variR = 64^(1/6) = 2 (64 in
         2D) throughout: 0.95 < 0.95 is false -> 3
      4  r falls 10 % every phase -> the loop's end, 11
      5  tiny spreads at phases 0 and 1 (before min_phase they do not count),
         then constant -> 3
      6  r falls 2 % a phase (4 % in 2D): never below 0.95 of the best -> 3
      7  k1 = 1 at phase 2, 0.95 at phase 3, k2 = k3 = 1: exactly no room in
         2D, and 0.95^(1/6) is no 5 % decrease in 3D -> 3
      8  only the defocus spread falls, 10 % a phase up to phase 5 -> 3
         without the criterion, 6 with it
      9  the defocus spread exactly 1 then exactly 0.95 -> 3 either way"""
    nPh, n = 12, 10
    r, s0, dd = np.ones((nPh, n)), np.ones((nPh, n)), np.ones((nPh, n))
    p = np.arange(nPh, dtype=np.float64)
    r[8:, 0] = 0.01
    r[:, 1] = 0.9 ** np.minimum(p, 6)
    s0[:, 2] = 0.9 ** np.minimum(p, 5)
    s0[3:, 3] = 0.95
    r[:, 4] = 0.9 ** p
    r[:2, 5], s0[:2, 5] = 1e-3, 1e-3
    r[:, 6] = 0.98 ** p
    dd[:, 8] = 0.9 ** np.minimum(p, 5)
    dd[3:, 9] = 0.95
    k = np.repeat((r * r)[:, :, None], 3, axis=2)
    k[:, 3] = (64.0, 1.0, 1.0)
    k[:, 7] = 1.0
    k[3:, 7, 0] = 0.95
    sd = np.stack([s0, np.ones((nPh, n))], axis=2)
    sd[8:, 0] = 0.01
    nP = np.array([3, 7, 6, 3, 11, 3, 3, 3, 3, 3], np.int32)
    nP_d = nP.copy()
    nP_d[8] = 6
    return k, sd, dd, nP, nP_d


def compact(n_img, done=None, order=None):
    """The images with done == 0, rising or in the order `order` lists them."""
    idx = np.arange(n_img) if order is None else np.asarray(order)
    return idx[done[idx] == 0] if done is not None else idx
