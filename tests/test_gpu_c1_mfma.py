"""Class 1's row sweeps as broadcast MFMA outer products (cmpc_class1.hip, mfma_chunk).

The Cholesky's trailing sweep and the active set's reflection update take the broadcast column
from lane c's register through v_mfma_f32_4x4x1_16b_f32 (cbsz 4, abid = c / 4) instead of from an
LDS broadcast. What can go wrong is the register layout the kernel assumes, and a chunk, pivot or
lane that the sweep misses at some reduced size n:

  * the probe (cmpc_mfma_probe, a child process of its own) checks the layout for every abid in
    every lane and register against fmaf;
  * class-1 batches at N = 1, 3, 5 and 10 with every contact random hold every reduced size
    n = 3, 6, ..., 63 and an n = 0 instance: every residue of n mod 4 (the last chunk partly
    identity padding), odd n (the last pair step's second pivot is the padding row), n = 60 and
    n = 61..63 (the columns only the 64-wide build has). The test asserts that on the inputs
    before it compares, so a change of the instance generator fails here instead of passing
    vacuously. Seed 7400 is the first of a search from 7400 on the CPU (reduced sizes are a
    function of the contact table alone). Batches below 16384 instances run the 64-wide build;
    the 60-wide one is held to it bit for bit by test_gpu_parity.py's test_batch_size_invariance;
  * a stressed N = 10 batch (test_gpu_active_set_paths.py's seed 7300, its first 512 instances,
    the class-1 ones of them) holds a class-1 instance with a drop (the reflection with beta = 0
    and the Givens chain after MFMA-updated rows) and one whose active set passes QI.

Forces are held to the live reference pipeline by test_gpu_parity.py's rule (1e-4).
"""
import json
import os
import subprocess

import numpy as np
import pytest

from support import active_counts, gpu_solve, solver_mod  # noqa: F401
from test_gpu_parity import assert_failed_reference, assert_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "quad-periodic-mpc_amd", "cmpc_mfma_probe")

SEED = 7400
CASES = [(1, 256), (3, 256), (5, 512), (10, 512)]   # (N, instances drawn; the class-1 ones are kept)
QI_64 = 45   # positions up to which the 64-wide build keeps R^-1 (SharedC1<64>::QI)


def class1_batch(cm, N, B, seed, stress=False):
    recs = cm.make_instances(B, N, seed=seed, stress=stress, random_contact_frac=1.0)
    n = 3 * (cm.unpack_gait(recs, N) != 0).sum(1)
    keep = n <= 64
    return np.ascontiguousarray(recs[keep]), n[keep]


def test_mfma_probe_layout():
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[mfma] probe: {d}")
    assert d["layout_ok"] is True, d


@pytest.fixture(scope="module")
def size_batches(cm):
    """{N: (records, n)} of CASES, made once; asserted to hold every reduced size together before
    any of them is compared."""
    out = {N: class1_batch(cm, N, B, SEED) for N, B in CASES}
    sizes = set()
    for N, (recs, n) in out.items():
        assert 256 <= len(recs) <= 512, (N, len(recs))
        sizes |= set(np.unique(n).tolist())
    want = set(range(0, 64, 3))   # n = 0 and every n = 3, 6, ..., 63
    assert sizes >= want, ("reduced sizes missing from the batches", sorted(want - sizes))
    return out


@pytest.mark.parametrize("N", [N for N, _ in CASES], ids=[f"n{N}" for N, _ in CASES])
def test_every_reduced_size_matches_reference_live(cm, orc, solver_mod, size_batches, N):
    prm = cm.make_params(N)
    recs, n = size_batches[N]
    f, st, it = gpu_solve(solver_mod, prm, recs)
    print(f"[mfma] N={N}: {len(recs)} class-1 instances, n in {sorted(np.unique(n).tolist())}, trips "
          f"mean {it.mean():.2f} max {it.max()}")
    assert (f[n == 0] == 0.0).all() and (st[n == 0] == 0).all()
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label=f"mfma sizes seed={SEED}")
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label=f"mfma sizes N={N}")


def test_drop_and_past_qi_after_mfma_rows_live(cm, orc, solver_mod):
    N = 10
    prm = cm.make_params(N)
    recs, n = class1_batch(cm, N, 512, 7300, stress=True)
    f, st, it = gpu_solve(solver_mod, prm, recs)
    _, hi, lo = active_counts(cm, prm, recs, f)
    solved = st == 0
    drops = int((solved & (it > hi)).sum())
    past = int((solved & (lo > QI_64)).sum())
    print(f"[mfma] stressed N=10: {len(recs)} class-1 instances, {drops} with a drop, {past} past QI, "
          f"trips mean {it.mean():.2f} max {it.max()}")
    assert drops >= 1, "no class-1 instance with a drop"
    assert past >= 1, "no class-1 instance whose active set passes QI"
    if not orc.ref_available():
        pytest.skip("oracle/_ref not present")
    q, st_ref, _ = orc.ref_solve_batch(recs, prm, nthreads=16)
    ok = st_ref == 0
    assert (st[ok] == 0).all(), np.bincount(st[ok])
    assert_parity(orc, recs, prm, f, q, ok, label="mfma stress=True frac=1.0")
    assert_failed_reference(orc, recs, prm, f, st, st_ref, label="mfma stress N=10")
