"""CPU-side checks of the table loader (csrc/load.hip thx_pf_load, csrc/
round.hip thx_pf_score, thunder_amd/table.py): both entry points reject bad
arguments with THX_ERR_ARG and a message before any device work, an empty
batch is a no-op, the Python front end refuses bad table rows by name, and a
round's table survives the file (%18.9f: half a unit is 5e-10)."""
import ctypes
import os

import numpy as np
import pytest

from thunder_amd import _lib, build, io, table

OK, BAD = 0, 1
d = ctypes.c_void_p(4096)
NEW = ("thx_pf_load", "thx_pf_score")
NUMERIC = [c for c in io.THU_COLUMNS if c not in io._THU_STR]


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def rejected(L, status):
    return status == BAD and len(L.thx_last_error()) > 0


def test_library_exposes_the_new_symbols(L):
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.thx_abi_version() == 9


def test_pf_load_validates_without_gpu(L):
    def call(n=5, mR=9, mT=9, mD=1, q=d, k=d, t=d, sd=d, dfo=(d, d, d, d), quat=d, trans=d,
             pR=d, pT=d, vari=d):
        topD, sdD, dd, pD = dfo
        return L.thx_pf_load(n, mR, mT, mD, q, k, t, sd, topD, sdD, 7, 0, quat, trans, pR, pT, dd,
                             pD, vari, None)

    none4 = (None, None, None, None)
    assert rejected(L, call(n=-1)) and b"nImg" in L.thx_last_error()
    for bad in ({"mR": 0}, {"mR": -3}, {"mT": 0}, {"mT": -1}, {"mD": -1}):
        assert rejected(L, call(**bad)), bad
    for name in ("q", "k", "t", "sd", "quat", "trans", "pR", "pT"):     # every required pointer
        assert rejected(L, call(**{name: None})), name
        assert b"null" in L.thx_last_error()
    for hole in range(4):                                   # the defocus group given in part
        part = tuple(None if j == hole else d for j in range(4))
        assert rejected(L, call(dfo=part)), hole
        only = tuple(d if j == hole else None for j in range(4))
        assert rejected(L, call(dfo=only, mD=0)), hole
    assert rejected(L, call(mD=0))                          # given, but no defocus samples
    assert rejected(L, call(mD=3, dfo=none4))               # samples, but nowhere to put them
    assert b"mD" in L.thx_last_error()
    # an empty batch: nothing to draw, whatever the pointers
    assert call(n=0) == OK
    assert call(n=0, mD=0, q=None, k=None, t=None, sd=None, dfo=none4, quat=None, trans=None,
                pR=None, pT=None, vari=None) == OK
    assert rejected(L, call(n=0, mR=0))                     # the sizes are checked even then


def test_pf_score_validates_without_gpu(L):
    assert rejected(L, L.thx_pf_score(-1, d, 0, d, None))
    assert rejected(L, L.thx_pf_score(4, None, 0, d, None))
    assert rejected(L, L.thx_pf_score(4, d, 0, None, None))
    assert rejected(L, L.thx_pf_score(4, d, 2, d, None))
    assert L.thx_pf_score(0, None, 0, None, None) == OK
    assert L.thx_pf_score(0, None, 1, None, None) == OK


# ------------------------------------------------------------------ the table
def good_table(n, seed=1):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = io.thu_table(n, [f"{i + 1:06d}@stack.mrcs" for i in range(n)], quat=q,
                     trans=rng.standard_normal((n, 2)) * 3)
    for name in ("k1", "k2", "k3"):
        t[name] = rng.uniform(1e-4, 1e-2, n)
    t["stdTransX"], t["stdTransY"] = rng.uniform(0.5, 2, n), rng.uniform(0.5, 2, n)
    t["stdDefocusFactor"] = rng.uniform(0, 0.01, n)
    t["score"] = rng.uniform(1, 10, n)
    return t


@pytest.mark.parametrize("column, value, word", [
    ("quat2", np.nan, "quat2 is not finite"), ("k1", np.inf, "k1 is not finite"),
    ("transY", -np.inf, "transY is not finite"), ("defocusFactor", np.nan, "defocusFactor"),
    ("stdDefocusFactor", np.nan, "stdDefocusFactor"),
    ("quat0", 3.0, "unit norm"),
    ("k1", 0.0, "k1 <= 0"), ("k2", -1e-3, "k2 <= 0"), ("k3", 0.0, "k3 <= 0"),
    ("stdTransX", -1.0, "stdTransX is negative"), ("stdTransY", -1e-9, "stdTransY is negative"),
    ("stdDefocusFactor", -0.5, "stdDefocusFactor is negative")])
def test_bad_rows_are_named(column, value, word):
    """The row is refused on the host table, before a device is touched."""
    t = good_table(7)
    t[column][4] = value
    with pytest.raises(ValueError, match="table row 4: .*" + word):
        table.particles_from_table(t, 125, 9)
    with pytest.raises(ValueError, match="table row 4"):     # through a shard's row list too
        table.particles_from_table(t, 125, 9, rows=[6, 4, 1])
    table.check_rows(t, rows=[0, 1, 2, 3, 5, 6])             # the other rows are fine


def test_quaternion_norm_bar_and_zero_spreads():
    t = good_table(3)
    q = np.stack([t[f"quat{j}"] for j in range(4)], axis=1)
    for j in range(4):
        t[f"quat{j}"] = q[:, j] * (1 + 5e-7)                 # inside the bar: taken as read
    t["stdTransX"][:] = 0.0                                  # sd = 0 is legal (the floors)
    t["stdDefocusFactor"][:] = 0.0
    c, rows = table.check_rows(t)
    assert np.array_equal(c[:, 0:4], q * (1 + 5e-7)) and list(rows) == [0, 1, 2]
    for j in range(4):
        t[f"quat{j}"] = q[:, j] * (1 + 2e-6)
    with pytest.raises(ValueError, match="table row 0: .*unit norm"):
        table.check_rows(t)
    with pytest.raises(ValueError, match="rows outside"):
        table.check_rows(good_table(3), rows=[3])


def test_2d_request_is_refused_with_the_reason():
    with pytest.raises(ValueError, match="MODE_2D"):
        table.particles_from_table(good_table(3), 125, 9, mode="2d")


def round_values(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    vari = np.concatenate([rng.uniform(1e-5, 1e-1, (n, 3)), rng.uniform(0.1, 3, (n, 2)),
                           rng.uniform(0, 0.02, (n, 1))], axis=1)
    return {"cls": rng.integers(0, 4, n).astype(np.int32), "quat": q,
            "trans": rng.standard_normal((n, 2)) * 2, "d": 1 + 0.05 * rng.standard_normal(n),
            "vari": vari, "offS": rng.standard_normal((n, 2)) * 4,
            "score": (vari[:, 0] * vari[:, 1] * vari[:, 2]) ** (-1.0 / 6)}


def check_round_columns(got, t, v, rows=slice(None)):
    """Every numeric column of the file `got` against what saveDatabase prints."""
    want = {"classID": v["cls"], "k1": v["vari"][:, 0], "k2": v["vari"][:, 1], "k3": v["vari"][:, 2],
            "transX": v["trans"][:, 0] - v["offS"][:, 0], "transY": v["trans"][:, 1] - v["offS"][:, 1],
            "stdTransX": v["vari"][:, 3], "stdTransY": v["vari"][:, 4],
            "defocusFactor": v["d"] if v["d"] is not None else np.asarray(t["defocusFactor"])[rows],
            "stdDefocusFactor": v["vari"][:, 5], "score": v["score"]}
    for j in range(4):
        want[f"quat{j}"] = v["quat"][:, j]
    worst = 0.0
    for name in NUMERIC:
        w = np.asarray(want.get(name, np.asarray(t[name])[rows]), np.float64)
        err = np.abs(np.asarray(got[name], np.float64) - w).max()
        worst = max(worst, err)
        assert err <= 5e-10, (name, err)
    return worst


@pytest.mark.parametrize("with_d", [True, False])
def test_round_table_survives_the_file(tmp_path, with_d):
    n = 11
    t = good_table(n, seed=5)
    t["coordinateX"], t["coordinateY"] = np.arange(n) * 10.5, np.arange(n) * -3.25
    t["groupID"] = np.arange(n) % 3 + 1
    v = round_values(n, 6)
    if not with_d:
        v["d"] = None
    out = table.round_table(t, v["cls"], v["quat"], v["trans"], v["d"], v["vari"], v["offS"],
                            score=v["score"])
    assert out is not t and np.array_equal(t["classID"], np.zeros(n))      # the input is left alone
    path = table.save_database(str(tmp_path) + os.sep, out, it=7)
    assert os.path.basename(path) == "Meta_Round_007.thu"
    got = io.read_thu(path)
    print("round trip: worst column error", check_round_columns(got, t, v))
    assert got["particlePath"] == t["particlePath"] and got["micrographPath"] == t["micrographPath"]
    final = table.save_database(str(tmp_path) + os.sep, out, finished=True)
    assert os.path.basename(final) == "Meta_Final.thu"
    assert open(final).read() == open(path).read()
    with pytest.raises(ValueError):
        table.save_database(str(tmp_path) + os.sep, out)
    with pytest.raises(ValueError, match="quat has shape"):
        table.round_table(t, v["cls"], v["quat"][:-1], v["trans"], v["d"], v["vari"], v["offS"],
                          score=v["score"])


def _gloo_rank(rank, world, port, prefix):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                            world_size=world)
    try:
        n = 5 + 2 * rank                                    # ranks hold different numbers of rows
        t = good_table(n, seed=20 + rank)
        t["particlePath"] = [f"{i + 1:06d}@rank{rank}.mrcs" for i in range(n)]
        v = round_values(n, 30 + rank)
        out = table.round_table(t, v["cls"], v["quat"], v["trans"], v["d"], v["vari"], v["offS"],
                                score=v["score"])
        table.save_database(prefix, out, it=3, group=dist.group.WORLD)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_save_database_gathers_in_rank_order(tmp_path):
    """Two gloo ranks with 5 and 7 rows: one file, rank 0's rows first -- what
    the reference's rank-by-rank append leaves."""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    prefix = str(tmp_path) + os.sep
    mp.spawn(_gloo_rank, args=(2, port, prefix), nprocs=2, join=True)
    got = io.read_thu(prefix + "Meta_Round_003.thu")
    assert got["particlePath"] == [f"{i + 1:06d}@rank0.mrcs" for i in range(5)] + \
        [f"{i + 1:06d}@rank1.mrcs" for i in range(7)]
    at = 0
    for rank, n in ((0, 5), (1, 7)):
        t, v = good_table(n, seed=20 + rank), round_values(n, 30 + rank)
        part = {name: np.asarray(got[name])[at:at + n] for name in NUMERIC}
        check_round_columns(part, t, v)
        at += n
