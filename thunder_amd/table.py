"""From a .thu table to the device particle state of a local search and back:
Optimiser::loadParticles -> Particle::load (src/Optimiser.cpp:452-497,
5312-5384; src/Particle.cpp:401-556) and Optimiser::saveDatabase
(src/Optimiser.cpp:8250-8416), over thx_pf_load (csrc/load.hip) and
thx_pf_score (csrc/round.hip).  The reference's only checkpoint / resume
mechanism: with ``Global Search = false`` a run starts from the pose and the
spreads of every table row, and every round ends by writing such a table.

    t = io.read_thu("Meta_Round_012.thu")
    loaded = table.particles_from_table(t, mLR=125, mLT=9, seed=7, device=dev)
    offS = table.start_local_search(stack, loaded, remask=(r_mask, edge))
    e = Expectation(vol, px, None, search="local")
    e.run(dat, ctf, sig, state=loaded.state)
    cls, quat, trans, d, vari = e.rank1st()
    out = table.round_table(t, cls, quat, trans, d, vari, offS)
    table.save_database(prefix, out, it=13)
"""
from collections import namedtuple

import numpy as np
import torch

from . import io
from . import round as rnd
from ._lib import check, lib
from .ops import _ptr, _req, _stream

# state: (quat [n, mLR, 4], trans [n, mLT, 2], pR [n, mLR], pT [n, mLT], cls [n])
#        for Expectation.run(state=...) / run_ctf;
# top:   (quat [n, 4], trans [n, 2], d [n]) -- Particle::_topR / _topT / _topD;
# vari:  [n, 6] k1 k2 k3 s0 s1 sD of the drawn clouds;  score: the table's column;
# defocus: (d [n, mLD], pD [n, mLD]), None with mLD = 0
Loaded = namedtuple("Loaded", "state top vari score defocus")

_LOAD_COLUMNS = ("quat0", "quat1", "quat2", "quat3", "k1", "k2", "k3", "transX", "transY",
                 "stdTransX", "stdTransY", "defocusFactor", "stdDefocusFactor")


def _host(x, dtype=np.float64):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype)


def check_rows(table, rows=None):
    """The host-side validation of particles_from_table: the columns
    Particle::load reads, as one [n, 13] float64 array in _LOAD_COLUMNS'
    order.  ValueError naming the table row for a non-finite value,
    | |quat| - 1 | > 1e-6, a k <= 0 or a negative standard deviation."""
    n_all = len(table["particlePath"])
    rows = np.arange(n_all) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= n_all):
        raise ValueError(f"rows outside the table's {n_all} rows")
    c = np.stack([np.asarray(table[name], np.float64)[rows] for name in _LOAD_COLUMNS], axis=1)

    def fail(bad, why):
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"table row {int(rows[i])}: {why}")

    finite = np.isfinite(c)
    for j, name in enumerate(_LOAD_COLUMNS):
        fail(~finite[:, j], f"{name} is not finite")
    fail(np.abs(np.linalg.norm(c[:, 0:4], axis=1) - 1.0) > 1e-6,
         "the quaternion is not of unit norm (| |quat| - 1 | > 1e-6)")
    for j in (4, 5, 6):
        fail(c[:, j] <= 0, f"{_LOAD_COLUMNS[j]} <= 0 (the ACG spread of a loaded rotation is positive)")
    for j in (9, 10, 12):
        fail(c[:, j] < 0, f"{_LOAD_COLUMNS[j]} is negative")
    return c, rows


def pf_score(vari, two_d=False):
    """thx_pf_score: Particle::compressR of every image from vari [n, 6]
    (device float64): (k1 k2 k3)^(-1/6), 2D: 1 / k1."""
    n = vari.shape[0]
    _req(vari, torch.float64, (n, 6), "vari")
    score = torch.empty(n, dtype=torch.float64, device=vari.device)
    check(lib().thx_pf_score(n, _ptr(vari), int(bool(two_d)), _ptr(score), _stream(vari.device)),
          "thx_pf_score")
    return score


def pf_load(top_quat, k, top_trans, sd, mLR, mLT, top_d=None, sd_d=None, mLD=0, seed=7,
            stream_id=0, want_vari=True):
    """thx_pf_load on device rows top_quat [n, 4], k [n, 3], top_trans [n, 2],
    sd [n, 2] (and top_d [n], sd_d [n] with mLD > 0), all float64: returns
    (quat, trans, pR, pT, d, pD, vari); d, pD None with mLD = 0, vari None
    unless wanted."""
    n = top_quat.shape[0]
    dev = top_quat.device
    _req(top_quat, torch.float64, (n, 4), "top_quat")
    _req(k, torch.float64, (n, 3), "k")
    _req(top_trans, torch.float64, (n, 2), "top_trans")
    _req(sd, torch.float64, (n, 2), "sd")
    if mLR <= 0 or mLT <= 0 or mLD < 0:
        raise ValueError("pf_load: mLR and mLT must be positive, mLD not negative")
    if mLD > 0:
        _req(top_d, torch.float64, (n,), "top_d")
        _req(sd_d, torch.float64, (n,), "sd_d")
    elif top_d is not None or sd_d is not None:
        raise ValueError("pf_load: top_d / sd_d without defocus samples (mLD = 0)")
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    quat, trans, pR, pT = new(n, mLR, 4), new(n, mLT, 2), new(n, mLR), new(n, mLT)
    d, pD = (new(n, mLD), new(n, mLD)) if mLD > 0 else (None, None)
    vari = new(n, 6) if want_vari else None
    check(lib().thx_pf_load(n, mLR, mLT, mLD, _ptr(top_quat), _ptr(k), _ptr(top_trans), _ptr(sd),
                            _ptr(top_d), _ptr(sd_d), int(seed), int(stream_id), _ptr(quat),
                            _ptr(trans), _ptr(pR), _ptr(pT), _ptr(d), _ptr(pD), _ptr(vari),
                            _stream(dev)), "thx_pf_load")
    return quat, trans, pR, pT, d, pD, vari


def particles_from_table(table, mLR, mLT, mLD=1, seed=7, stream_id=0, device="cuda:0", rows=None,
                         mode="3d"):
    """Optimiser::loadParticles: the particle state of every row of `table`
    (io.read_thu; rows: the indices this process owns, default all) around the
    row's pose with the row's spreads (thx_pf_load).  Returns Loaded(state,
    top, vari, score, defocus); state's cls is 0 as Particle::load sets it
    (substitute the table's classID where the classes are kept).  Quaternions
    are passed on as read: the reference does not renormalise them.
    Image l of the returned batch draws from the counter streams
    (seed; l, stream_id, .): ranks that share a seed pass distinct stream_ids."""
    if mode != "3d":
        raise ValueError("particles_from_table: MODE_3D tables only -- Particle::load has no "
                         "MODE_2D form (it draws 4-D ACG rotations whatever the mode), so a 2D "
                         "table cannot seed a 2D search's (cos, sin, 0, 0) rotations")
    c, rows = check_rows(table, rows)
    dev = torch.device(device)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    top_q, k, top_t, sd = up(c[:, 0:4]), up(c[:, 4:7]), up(c[:, 7:9]), up(c[:, 9:11])
    top_d, sd_d = up(c[:, 11]), up(c[:, 12])
    quat, trans, pR, pT, d, pD, vari = pf_load(top_q, k, top_t, sd, mLR, mLT,
                                               top_d if mLD > 0 else None,
                                               sd_d if mLD > 0 else None, mLD, seed, stream_id)
    cls = torch.zeros(len(rows), dtype=torch.int32, device=dev)
    score = up(np.asarray(table["score"], np.float64)[rows])
    return Loaded((quat, trans, pR, pT, cls), (top_q, top_t, top_d), vari, score,
                  (d, pD) if mLD > 0 else None)


def start_local_search(stack, loaded, remask=None):
    """What Optimiser::init does after loadParticles (src/Optimiser.cpp:466-496):
    reCentreImg with the loaded top translation -- stack.imgFT <- stack.oriFT
    shifted, the translation cloud and the top moved to the new origin -- then
    reMaskImg when remask = (rMask, edge).  Returns the images' offsets offS
    [n, 2] (= -the table's translation), which the insert and round_table take."""
    top_t = loaded.top[1]
    offS = torch.zeros_like(top_t)
    rnd.recentre(stack.oriFT, stack.imgFT, top_t, offS, trans=loaded.state[1], remask=remask)
    return offS


def grading_weights(vari, m_reco, grade=True, two_d=False):
    """The per-image insert weight w [n] float32 of ops.insert3d:
    compressR() / mReco with _para.parGra (src/Optimiser.cpp:6762-6763,
    6972-6977), else 1 / mReco."""
    if m_reco <= 0:
        raise ValueError("grading_weights: m_reco must be positive")
    if not grade:
        return torch.full((vari.shape[0],), 1.0 / m_reco, dtype=torch.float32, device=vari.device)
    return (pf_score(vari, two_d) / m_reco).float()


def round_table(table, cls, quat, trans, d, vari, offS, score=None, two_d=False):
    """The rows saveDatabase prints (src/Optimiser.cpp:8365-8405) for the
    images of `table` (the process's own rows, in order): classID, quat, k1-3,
    stdTransX/Y and stdDefocusFactor from Expectation.rank1st(), transX/Y =
    trans - offS (OPTIMISER_RECENTRE_IMAGE_EACH_ITERATION), defocusFactor = d
    (the table's own value where no CTF search ran: d None), score =
    compressR (thx_pf_score on the device vari) unless given.  Every other
    column is the table's.  Returns a new table; tensors or arrays are taken."""
    n = len(table["particlePath"])
    if score is None:
        score = pf_score(vari, two_d)
    q, t, v, off = _host(quat), _host(trans), _host(vari), _host(offS)
    for name, a, shape in (("quat", q, (n, 4)), ("trans", t, (n, 2)), ("vari", v, (n, 6)),
                           ("offS", off, (n, 2))):
        if a.shape != shape:
            raise ValueError(f"round_table: {name} has shape {a.shape}, expected {shape}")
    out = {name: (list(col) if name in io._THU_STR else np.array(col)) for name, col in table.items()}
    out["classID"] = _host(cls, np.int64).reshape(n)
    for j in range(4):
        out[f"quat{j}"] = q[:, j].copy()
    out["k1"], out["k2"], out["k3"] = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
    out["transX"], out["transY"] = t[:, 0] - off[:, 0], t[:, 1] - off[:, 1]
    out["stdTransX"], out["stdTransY"] = v[:, 3].copy(), v[:, 4].copy()
    if d is not None:
        out["defocusFactor"] = _host(d).reshape(n)
    out["stdDefocusFactor"] = v[:, 5].copy()
    out["score"] = _host(score).reshape(n)
    return out


def database_path(prefix, it=None, finished=False):
    if finished:
        return f"{prefix}Meta_Final.thu"
    if it is None:
        raise ValueError("save_database: a round number, or finished=True")
    return "%sMeta_Round_%03d.thu" % (prefix, it)


def save_database(prefix, table, it=None, finished=False, group=None):
    """saveDatabase: write Meta_Round_%03d.thu (it) or Meta_Final.thu through
    io.write_thu.  With a torch.distributed group every rank passes its own
    rows; they are gathered to the group's first rank in rank order and
    written once -- the file the reference's rank-by-rank append produces.
    Collective over the group.  Returns the path (on every rank)."""
    import torch.distributed as dist
    path = database_path(prefix, it, finished)
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        io.write_thu(path, table)
        return path
    first = dist.get_global_rank(group, 0) if group is not None else 0
    me = dist.get_rank()
    parts = [None] * dist.get_world_size(group) if me == first else None
    dist.gather_object(table, parts, dst=first, group=group)
    if me == first:
        whole = {}
        for name in io.THU_COLUMNS:
            cols = [p[name] for p in parts]
            whole[name] = sum((list(c) for c in cols), []) if name in io._THU_STR else \
                np.concatenate([np.asarray(c) for c in cols])
        io.write_thu(path, whole)
    return path
