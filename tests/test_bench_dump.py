"""bench.py --dump-outputs / --full on the host: the dump writes Expectation.run's
tuple as float32 / float64 .npy files, whole when it fits the byte budget and
the same seeded rows of every array when it does not; a plain run asks for
none of the extra measurements."""
import os
import sys

import numpy as np
import torch

import bench


def _outs(n, mR=125, mT=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, mR, 4, dtype=torch.float64, generator=g),
            torch.randn(n, mT, 2, dtype=torch.float64, generator=g),
            torch.rand(n, mR, dtype=torch.float64, generator=g),
            torch.rand(n, mT, dtype=torch.float64, generator=g),
            torch.randn(n, dtype=torch.float32, generator=g),
            torch.zeros(n, dtype=torch.int32),
            torch.full((n,), 10, dtype=torch.int32))


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_whole_over_sub_batches(tmp_path):
    a, b = _outs(5, seed=1), _outs(3, seed=2)
    bench.dump_outputs([a, b], str(tmp_path / "d"))
    d = _load(tmp_path / "d")
    assert sorted(d) == sorted(bench.DUMP_NAMES + ("image_index",))
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert np.array_equal(d["image_index"], np.arange(8))
    for k, name in enumerate(bench.DUMP_NAMES):
        assert np.array_equal(d[name], torch.cat([a[k], b[k]]).numpy().astype(d[name].dtype)), name
    assert d["quat"].shape == (8, 125, 4) and d["score"].dtype == np.float32


def test_dump_samples_the_same_rows_past_the_budget(tmp_path, monkeypatch):
    o = _outs(40)
    per_image = 125 * 4 * 8 + 9 * 2 * 8 + 125 * 8 + 9 * 8 + 4 + 8 + 8 + 8
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * per_image + 100)
    bench.dump_outputs([o], str(tmp_path / "a"))
    bench.dump_outputs([o], str(tmp_path / "b"))
    d, d2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    idx = d["image_index"].astype(np.int64)
    assert len(idx) == 10 and np.all(np.diff(idx) > 0) and idx[-1] < 40
    assert sum(v.nbytes for v in d.values()) <= bench.DUMP_BYTES
    for k, name in enumerate(bench.DUMP_NAMES):
        assert np.array_equal(d[name], o[k].numpy()[idx].astype(d[name].dtype)), name
        assert np.array_equal(d[name], d2[name])


def test_bench_batch_dump_fits_64_mb():
    """The headline batch (12 500 images, 125 x 9 clouds) is sampled below 64 MB."""
    per_image = 125 * 4 * 8 + 9 * 2 * 8 + 125 * 8 + 9 * 8 + 4 + 8 + 8 + 8
    assert 12500 * per_image > bench.DUMP_BYTES
    assert bench.DUMP_BYTES // per_image * per_image + 8 * 128 <= 64 * 10 ** 6


def test_plain_run_measures_nothing_else(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (4, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
