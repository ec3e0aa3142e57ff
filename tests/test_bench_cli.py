"""bench.py's command line: a plain run is the headline alone, --full adds the other measurements,
--dump-outputs writes the last timed step's outputs and is reproducible run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FILES = ("binds_pod", "binds_node", "binds_status", "binds_tick", "usage")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels", "usage_query", "dropin", "c3q", "c3_literal", "c4", "c5_sharded",
             "cpu_baseline")


def _bench_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_options_present():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


def test_dump_outputs_files(tmp_path):
    """The dump is float64, exact for the engine's integers, and a large array is cut to the same
    seeded sample every time."""
    bench = _bench_module()
    dt = np.dtype([("pod", "<i8"), ("node", "<i4"), ("status", "<i4"), ("tick", "<i8")])
    binds = np.zeros(5, dt)
    binds["pod"] = np.arange(5) + (1 << 40)
    binds["node"] = [3, 1, 4, 1, 5]
    binds["tick"] = np.arange(5) + 7
    usage = np.arange((1 << 20) + 10, dtype=np.int64).repeat(3).reshape(-1, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), binds, usage)
    for name in FILES:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and (a == b).all()
    assert (np.load(tmp_path / "a" / "binds_pod.npy") == binds["pod"]).all()
    assert (np.load(tmp_path / "a" / "binds_node.npy") == binds["node"]).all()
    u = np.load(tmp_path / "a" / "usage.npy")
    assert u.shape == (1 << 20, 3) and (np.diff(u[:, 0]) > 0).all()  # a sample of rows, in order
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in FILES) <= 64 << 20


def _run(args):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--nodes", "2000", "--pods", "4000",
                        "--pods-per-step", "512"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]  # one JSON result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_reproducibly(tmp_path):
    """A small C3-shaped cluster, 3 timed steps: the line holds the headline and none of the --full
    measurements; two runs with the same arguments dump identical arrays, and the dumped binds are
    the last timed step's (pods 3*512 .. 4*512 - 1, one per tick, on valid nodes)."""
    lines = [_run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        for k in HEADLINE:
            assert k in line, k
        for k in FULL_ONLY:
            assert k not in line, k
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "evals/s"
        assert line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "int64"
        # value = evals / s over the timed steps = binds x nodes / (steps x ms_per_step)
        assert line["value"] == pytest.approx(3 * 512 * 2000 / (3 * line["ms_per_step"] * 1e-3), rel=1e-9)
    out = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in FILES}
    for n in FILES:
        assert out[n].dtype == np.float64
        assert (out[n] == np.load(tmp_path / "b" / f"{n}.npy")).all(), n
    assert (out["binds_pod"] == np.arange(3 * 512, 4 * 512)).all()
    assert (np.diff(out["binds_tick"]) == 1).all()
    assert ((out["binds_node"] >= 0) & (out["binds_node"] < 2000)).all()
    assert out["usage"].shape == (2000, 3) and out["usage"].sum() > 0
