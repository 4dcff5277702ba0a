"""bench.py's sub-record workloads (CPU only): the c3r / c3rd records are the shipped plugin set without and with
reservations holding devices, and the full-size GPU parity test checks the c3rd record's own workload."""
import numpy as np

import bench
from koordinator_amd import synth


def test_c3r_holds_no_devices():
    w = bench.build_workload("c3r", seed=20261015, n_pods=500)
    assert w.reservations is not None and w.reservations.dev_allocatable is None


def test_c3rd_is_the_parity_tests_workload():
    w = bench.build_workload("c3rd", seed=20261015)
    ref = synth.c3_rsv(seed=20261015, dev_rsv_frac=0.7)  # tests/test_gpu_shipped_profile.py (full size)
    assert (w.nodes.n, w.pods.n) == (5000, 10_000)
    assert np.array_equal(w.reservations.dev_allocatable, ref.reservations.dev_allocatable)
    held = (w.reservations.dev_allocatable != 0).any(axis=1)
    assert 0.3 < held.mean() < 0.35


def test_dump_outputs_is_exact_and_bounded(tmp_path, monkeypatch):
    n = 300
    res = {"node": np.arange(n, dtype="<i4") - 1, "score": np.arange(n, dtype="<i8") * 10**12,
           "cpusets": np.full((n, 4), 2**63 + 5, np.uint64)}
    bench.dump_outputs(res, str(tmp_path / "all"))
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in res}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["node"].astype("<i4"), res["node"]) and np.array_equal(got["score"].astype("<i8"), res["score"])
    assert np.array_equal(got["cpusets"].astype("<u4").view(np.uint64), res["cpusets"])  # 32-bit halves, little-endian
    # above the size limit: one seeded sample of pod rows for every column, the same from run to run
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    for d in ("s1", "s2"):
        bench.dump_outputs(res, str(tmp_path / d))
    rows = np.load(tmp_path / "s1" / "rows.npy").astype(np.int64)
    assert 0 < len(rows) < n and np.array_equal(rows, np.load(tmp_path / "s2" / "rows.npy"))
    assert sum((tmp_path / "s1" / f).stat().st_size - 128 for f in ("rows.npy", "node.npy", "score.npy", "cpusets.npy")) <= 4000
    assert np.array_equal(np.load(tmp_path / "s1" / "score.npy"), res["score"][rows].astype(np.float64))
