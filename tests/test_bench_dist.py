"""bench.py's multi-rank path on CPU (gloo, plumbing stand-in for the solve): `--gpus N`
relaunches under torch.distributed.run, config 4 strong-scales the global batch over the ranks
with the root scatter -> solve -> gather pipeline, and the gathered per-instance rows are
bitwise identical to a world-size-1 run (per-instance seeds: every shard holds the instances a
1-GPU run holds)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _bench(*args, timeout=240):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "1",
                        "--warmup", "1", "--no-extras", *args],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus,gb,chunks", [(2, 262144, 4), (3, 10007, 3)])
def test_config4_sharded_equals_single(gpus, gb, chunks):
    one = _bench("--config", "4", "--global-batch", str(gb), "--chunks", str(chunks))
    many = _bench("--gpus", str(gpus), "--global-batch", str(gb), "--chunks", str(chunks))
    assert one["n_gpus"] == 1 and many["n_gpus"] == gpus
    assert many["config"]["config"] == 4 and many["scaling"] == "strong"
    assert one["config"]["global_batch"] == gb and many["config"]["global_batch"] == gb
    assert many["forces_digest"] == one["forces_digest"]
    assert many["status_counts"] == {"ok": gb}


def test_dump_outputs_of_a_plain_run(tmp_path):
    """--dump-outputs writes the last timed step's gathered forces as float32 .npy (the bytes the
    line's forces_digest hashes); a run without --full carries none of the extra legs."""
    import hashlib
    import numpy as np
    gb = 1000
    d = _bench("--config", "4", "--global-batch", str(gb), "--chunks", "2",
               "--dump-outputs", str(tmp_path / "out"))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["forces.npy"]
    f = np.load(tmp_path / "out" / "forces.npy")
    assert f.dtype == np.float32 and f.shape == (gb, 120)
    assert hashlib.sha256(f.tobytes()).hexdigest()[:16] == d["forces_digest"]
    assert d["dumped_outputs"]["instances"] == gb and not d["dumped_outputs"]["sampled"]
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None
    for k in ("solve_only", "end_to_end", "abi_latency", "other_configs", "scaling_model"):
        assert k not in d


def test_dump_outputs_samples_fixed_rows(tmp_path, monkeypatch):
    """Outputs beyond the size budget: the same seeded rows of every array, listed in rows.npy."""
    import numpy as np
    import torch
    import bench
    B = 1000
    forces = torch.arange(B * 24, dtype=torch.float32).reshape(B, 24)
    iters = torch.arange(B, dtype=torch.int32)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10000)
    info = [bench.dump_outputs(str(tmp_path / n), {"forces": forces, "iters": iters}) for n in "ab"]
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert info[0]["sampled"] and info[0]["instances"] == len(rows) == 10000 // (25 * 4 + 8)
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < B
    r = rows.astype(np.int64)
    total = 0
    for name, t in (("forces", forces), ("iters", iters)):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, t.numpy()[r].astype(np.float32))
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
        total += a.nbytes
    assert total + rows.nbytes <= 10000


def test_weak_mode_shards_reproduce_ids(cm):
    """Per-rank generation of instance ids [r*B, (r+1)*B) equals slices of one generation."""
    import numpy as np
    full = cm.make_instances(300, 10)
    parts = [cm.make_instances(100, 10, first_id=100 * r) for r in range(3)]
    np.testing.assert_array_equal(np.concatenate(parts), full)
