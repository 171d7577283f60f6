"""bench.py's plain run, `--dump-outputs` and `--full`.

* `dump_array` (CPU): float64 files; an array above DUMP_CAP elements is cut to
  the same seeded, ordered sample on every call.
* a plain run (GPU, config 1's 10k ops): `--steps` timed steps, the headline
  keys and none of the `--full` measurements; the dumped result, replicas,
  document and canonical hashes equal what the same merge gives through
  crdtm.tree in this process.
* `--full` (GPU, same workload, CPU baseline and PMC child passes off): the
  per-kernel roofline rides along and the headline keys keep their meaning.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
HEADLINE = {"metric": "merged ops/sec (whole node) on 10M-op batch", "unit": "ops/s", "higher_is_better": True,
            "dtype": "int64"}


def test_dump_array_sample(tmp_path):
    args = argparse.Namespace(dump_outputs=str(tmp_path / "d"))
    big = np.arange(bench.DUMP_CAP + 12345, dtype=np.uint32)
    bench.dump_array(args, 0, 1, "big", big)
    a = np.load(tmp_path / "d" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_CAP,)
    assert np.all(np.diff(a) > 0) and a[-1] < big.size  # distinct elements, in order
    bench.dump_array(args, 0, 1, "big", big)
    assert np.array_equal(np.load(tmp_path / "d" / "big.npy"), a)  # the same sample every time
    bench.dump_array(args, 1, 2, "small", [[1, 2], [3, 4]])
    s = np.load(tmp_path / "d" / "small_rank1.npy")
    assert s.dtype == np.float64 and s.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert 8 * bench.DUMP_CAP <= 32 << 20  # document + the small arrays stay under 64 MB


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "cfg1", "--steps", "3", "--warmup", "1",
                        *extra], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    for k, v in HEADLINE.items():
        assert line[k] == v, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    n = bench.WORKLOADS["cfg1"]["n_ops"]
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] / 1e3), rel=1e-9)  # ops of one step / its time
    return line


@pytest.mark.gpu
def test_plain_run_dumps_the_merge(tmp_path):
    from crdtm import _native as N
    from crdtm.tree import CRDTree
    line = run_bench("--dump-outputs", str(tmp_path))
    assert not {"roofline", "cpu_baseline", "exchange"} & set(line)
    assert "guard_g" not in line["config"] and "time_share" not in line["config"]["serial_replay"]
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["canonical", "document", "replicas", "result"]
    assert all(a.dtype == np.float64 for a in got.values())
    s = N.synth(**bench.WORKLOADS["cfg1"])
    n = len(s["kind"])
    t = CRDTree.init(0)
    res = t.apply_arrays(s, n)
    assert res.code == 0
    want = [res.code, res.path_taken, res.err_index, res.n_applied, res.n_already, res.timestamp, res.n_slots,
            res.guard, res.flags]
    assert got["result"].tolist() == [float(x) for x in want]
    assert got["replicas"].tolist() == [[float(r), float(ts)] for r, ts in sorted(t.replicas().items())]
    assert np.array_equal(got["document"], t.document_handles().astype(np.float64))
    for which in (0, 1):
        _, nw, h = t.canonical(which, full=False)
        assert got["canonical"][which].tolist() == [float(nw), float(h >> 32), float(h & 0xFFFFFFFF)]


@pytest.mark.gpu
def test_full_run_adds_the_roofline():
    line = run_bench("--full", "--cpu-sample", "0", "--pmc", "off")
    r = line["roofline"]
    assert r["top_kernels"] and r["dominant_kernel"]["name"] == r["top_kernels"][0]["name"]
    assert r["alg_bytes"] > 0 and r["achieved"] == pytest.approx(r["alg_bytes"] / (line["ms_per_step"] / 1e3) / 1e9)
    assert r["stream_copy_gbs"] > 0 and "time_share" in line["config"]["serial_replay"]
    assert "guard_g" in line["config"]
