"""bench.py's N-rank launch path on a machine without GPUs: `python bench.py --gpus 2 --dry-run` (no launcher, no
WORLD_SIZE in the environment — the way the driver may call it) must start two ranks by itself, shard the global batch
with `partition_molecules`, run one collective (gloo here; RCCL on the GPU box) and print ONE JSON line with n_gpus = 2."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    env["OMP_NUM_THREADS"] = "2"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


def test_self_launch_two_ranks_dry_run():
    line, err = _run(["--gpus", "2", "--dry-run", "--batch", "6", "--atoms", "12"])
    assert "re-executing under torch.distributed.run" in err
    assert line["n_gpus"] == 2 and line["dry_run"] is True
    assert line["every_molecule_owned_once"] is True
    assert sum(line["shard_sizes"]) == 12 and min(line["shard_sizes"]) >= 4    # balanced by triplet count
    assert line["collective"] == "gloo all_reduce"


def test_single_rank_dry_run_needs_no_launcher():
    line, err = _run(["--gpus", "1", "--dry-run", "--batch", "4", "--atoms", "12"])
    assert "re-executing" not in err
    assert line["n_gpus"] == 1 and line["shard_sizes"] == [4]


def test_dump_outputs_writes_float_arrays_within_the_size_limit(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: float32 arrays (float64 kept), and past the size limit a fixed seeded sample of rows that is
    the same in every run, stored with its row numbers."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"E": torch.randn(8, 1, generator=g), "F": torch.randn(256, 3, generator=g, dtype=torch.float64),
              "loss": torch.tensor(0.5), "params": torch.randn(20000, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32) and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.numpy().astype(a.dtype))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 65536)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(p.name for p in (tmp_path / "b").iterdir())
    assert files == ["E.npy", "F.npy", "loss.npy", "params.npy", "params_rows.npy"]
    assert sum((tmp_path / "b" / f).stat().st_size for f in files) <= 65536
    rows = np.load(tmp_path / "b" / "params_rows.npy").astype(np.int64)
    assert len(rows) > 0 and np.array_equal(np.load(tmp_path / "b" / "params.npy"), arrays["params"].numpy()[rows])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))
