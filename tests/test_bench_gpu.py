"""bench.py's command line on one GPU (Flickr-sized graph, a few steps): a plain run times
--steps steps and prints the headline line without the --full legs; --dump-outputs writes the
last step's outputs, the same from run to run; --full adds the checks and baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

V, D, K = 89250, 64, 16  # maxk_graph.PRESETS["flickr"]


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("MAXK_VALIDATE", None)  # the bench validates its graph once itself
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--graph",
                        "flickr", "--steps", "3", "--warmup", "1", *args],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    """One plain and one --full run with the same arguments, each dumping its outputs."""
    d = tmp_path_factory.mktemp("bench")
    plain = _bench("--dump-outputs", str(d / "plain"))
    full = _bench("--full", "--cpu-seconds", "0.5", "--dump-outputs", str(d / "full"))
    return plain, full, d


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(runs):
    d, _, tmp = runs
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "GTEPS" and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    # value and ms_per_step describe the same timed region: 2E edges per step
    assert d["value"] == pytest.approx(2 * d["config"]["E"] / d["ms_per_step"] / 1e6, rel=1e-2)
    # the --full legs stay out of a plain run
    assert d["cpu_baseline"] is None
    for key in ("adjoint_rel_err", "pull_locality", "topk_ms", "rocsparse_spmm_ms",
                "cpu_spmm_scipy"):
        assert key not in d["extra"], key
    for name, shape in (("y", (V, D)), ("gs", (V, K))):
        x, y = np.load(tmp / "plain" / f"{name}.npy"), np.load(tmp / "full" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == shape
        # every vertex has a self loop, so every row of either output holds something
        assert np.isfinite(x).all() and (x != 0).any(axis=1).mean() > 0.99
        # same arguments, same inputs: the runs differ by summation order at the most
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-5)
    assert sorted(os.listdir(tmp / "plain")) == ["gs.npy", "y.npy"]


@pytest.mark.gpu
def test_bench_full_run_keeps_its_legs(runs):
    _, d, _ = runs
    e = d["extra"]
    assert e["adjoint_rel_err"] <= 1e-6
    assert e["pull_locality"] > 0 and e["topk_ms"] > 0 and e["rocsparse_spmm_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and e["cpu_spmm_scipy"]["value"] > 0
