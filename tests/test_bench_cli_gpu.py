"""bench.py's command line: a plain run prints the result line with the headline fields and skips
what only ``--full`` measures; ``--dump-outputs`` writes the last timed step's arrays, identical
from run to run (seeded weights and batches). One tiny eager configuration, run twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "2", "--batch", "8", "--image-size", "64",
        "--graph", "off"]


def _run(out_dir):
    # heuristic tiles: at a shape outside the shipped tuning table the first-sight tuner would
    # time its candidates, and its pick (hence the rounding) could differ between the two runs
    env = dict(os.environ, LWAAAI_GEMM_TUNE="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS,
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True,
                       text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    a, b = tmp_path_factory.mktemp("dump_a"), tmp_path_factory.mktemp("dump_b")
    return _run(a), a, _run(b), b


@pytest.mark.gpu
def test_plain_result_line(runs):
    line = runs[0]
    assert line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 2 and line["warmup"] == 2
    assert line["ms_per_step"] > 0
    # images/s is the batch over the step time
    assert line["value"] == pytest.approx(8 * 1e3 / line["ms_per_step"], rel=1e-3)
    # what only --full measures is reported as not measured
    assert line["top1"] is None and line["comm"]["bucket_us"] is None


@pytest.mark.gpu
def test_dump_outputs_reproducible(runs):
    _, a, _, b = runs
    names = sorted(os.listdir(a))
    assert names == ["logits.npy", "loss.npy", "params_sample.npy"] == sorted(os.listdir(b))
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float32 and np.isfinite(x).all()
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 * 2**20
    assert np.load(os.path.join(a, "logits.npy")).shape == (8, 1000)
    assert np.load(os.path.join(a, "loss.npy")).shape == (1,)
