"""bench.py's command line: a plain run times the steps and nothing else,
--full adds the secondary measurements, --dump-outputs writes what the last
timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_within_its_budget(tmp_path, monkeypatch):
    """A batch over the budget is dumped for a sorted sample of its images,
    the same sample in every run; the per-image scalars stay whole."""
    import torch

    import bench
    monkeypatch.setattr(bench, "torch", torch)
    B, n, M1 = 10, 8, 5
    rng = np.random.default_rng(1)
    out = {"x": torch.from_numpy(rng.random((B, n, n))), "discr": torch.from_numpy(rng.random((B, M1))),
           "iters": torch.arange(B, dtype=torch.int32), "beta_final": torch.full((B,), 1.05).double()}
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 * (n * n + M1) * 8 + 7)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
        got.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert sorted(a) == ["beta_final", "discr", "images", "iters", "x"]
    assert all(v.dtype == np.float64 for v in a.values())
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["images"].astype(int)
    assert len(idx) == 3 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    np.testing.assert_array_equal(a["x"], out["x"].numpy()[idx])
    np.testing.assert_array_equal(a["discr"], out["discr"].numpy()[idx])
    np.testing.assert_array_equal(a["iters"], np.arange(B))
    assert sum(v.nbytes for k, v in a.items() if k in ("x", "discr")) <= bench.DUMP_BUDGET
    # under the budget: every image
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)
    bench.dump_outputs(str(tmp_path / "c"), out)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "images.npy"), np.arange(B))
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "x.npy"), out["x"].numpy())


def test_full_is_off_by_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 4
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """C3's shape at 8 images, MAXIT 3, one workgroup per image: the result
    line of a plain run carries the headline figures and none of --full's;
    the dump is the solve of the seeded inputs, bit for bit what a solve of
    the same generator's images returns in this process."""
    B, M, K = 8, 3, 2
    d = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                          str(K), "--warmup", "1", "--batch", str(B), "--maxit", str(M), "--team",
                          "1", "--dump-outputs", str(d)], capture_output=True, text=True,
                         timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == K and r["unit"] == "image-iterations/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f64" and r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(K * B * M / (r["ms_per_step"] * K / 1e3), rel=1e-9)
    assert r["roofline"] is None and r["cpu_baseline"] is None and "end_to_end" not in r
    a = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert sorted(a) == ["beta_final", "discr", "images", "iters", "x"]
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in a.values())
    np.testing.assert_array_equal(a["images"], np.arange(B))
    np.testing.assert_array_equal(a["iters"], np.full(B, M))
    assert a["x"].shape == (B, 256, 256) and a["discr"].shape == (B, M + 1)

    import torch

    import bench
    import sgp
    bench.torch = torch
    gn, psf = bench.synth_batch(B, 256, 25, 200, seed0=0)
    gn2, _ = bench.synth_batch(B, 256, 25, 200, seed0=0)
    assert torch.equal(gn, gn2)
    bkg = torch.full((B,), 100.0, dtype=torch.float64, device="cuda")
    here = sgp.sgp_betaDiv_batch(gn, psf, bkg, **bench.solve_kwargs(M, None, team=1))
    np.testing.assert_array_equal(here["x"], a["x"])
    np.testing.assert_array_equal(here["discr"], a["discr"])
