#!/usr/bin/env python3
"""Every output of the CTF-search driver (SEARCH_TYPE_CTF: quat, trans, pR, pT,
score, cls, nPhase, d, pD) on the workload of
tests/test_gpu_ctfsearch.py::test_ctf_search_driver_refines_defocus -- box 64,
rU 16, 128 images, 125 x 9 x 9 -- with 3 fixed phases and with the stopping
rule, saved as .npy under DIR to compare two libraries bit for bit
(tools/cmp_dump.py; the ctf3d row of profiles/local_phase_refactor_identity.jsonl).
    THX_LIB=... python tools/expect_dump_ctf.py DIR"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thunder_amd import expectation as ex, ops, synth  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
DEV = torch.device("cuda", 0)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


N, rU, n = 64, 16, 128
vol = synth.projectee(synth.blob_volume(N, seed=31, device=DEV), 2)
px = ops.PixelSet(N, 2, rU, 1, device=DEV)
rng = np.random.default_rng(32)
qtrue = synth.uniform_quaternions(n, rng)
ttrue = rng.standard_normal((n, 2))
attrs = synth.ctf_attrs(n, seed=33)
dtrue = 1 + rng.uniform(-0.03, 0.03, n)
a_true = attrs.copy()
a_true[:, 2:4] *= dtrue[:, None]
ctf = ops.ctf(T(a_true), px)
sigl = ctf * ops.project3d(vol, ops.rotmat(T(qtrue)), px) * ops.trans_table(T(ttrue), px)
dat, sig = synth.noisy_images(sigl, px.iSig, N // 2 + 1, snr=5.0, seed=34)
mR, mT = 125, 9
e0 = rng.standard_normal((n, mR, 4)) * np.radians(1.0) / 2
e0[..., 0] = 1.0
e0 /= np.linalg.norm(e0, axis=-1, keepdims=True)
w0, x0, y0, z0 = [qtrue[:, None, k] for k in range(4)]
w1, x1, y1, z1 = [e0[..., k] for k in range(4)]
quat = np.stack([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                 w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1], -1)
trans = ttrue[:, None, :] + rng.uniform(-0.5, 0.5, (n, mT, 2))
names = ("quat", "trans", "pR", "pT", "score", "cls", "nphase", "d", "pD")
for tag, kw in (("fixed", dict(n_phase=3)), ("converge", dict(converge=True))):
    state = (T(quat), T(trans), T(np.full((n, mR), 1.0 / mR)), T(np.full((n, mT), 1.0 / mT)))
    e = ex.Expectation(vol, px, None, search="ctf", seed=5, mLD=9, **kw)
    res = e.run_ctf(dat, T(attrs), sig, state)
    for name, x in zip(names, res):
        np.save(os.path.join(out, f"ctf3d_{tag}_{name}.npy"), x.cpu().numpy())
print("ok")
