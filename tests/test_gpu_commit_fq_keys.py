"""The slot-key table of the Fit + LoadAware + ElasticQuota commit kernel (ks_fq.h): the evaluator wave's keys (the
default when the table fits the commit's LDS image) against the CPU oracle and against the same library with
KS_FQ_KEYS=0 (wave 0 evaluates the touched slots itself; read when a context is created).  Compared: every result
column, the node state, the quota `used` table and the pass counters.

The shapes are those of test_gpu_commit_fq.py: 257 nodes (5 chunks, the last with one node), 130 pods (three passes,
the last with 2 pods; with passes of 7 pods the last has 4), 40 nodes for the cases that must reuse slots.
"""
import os

import numpy as np
import pytest

from helpers import assert_same_results, assert_same_state, homogeneous_pods, profile, stress_pods
from koordinator_amd import abi, synth
from koordinator_amd.config import (BATCH_CPU, BATCH_MEMORY, CPU, MEMORY, ElasticQuotaArgs, LoadAwareSchedulingArgs,
                                    NodeResourcesFitArgs, SchedulerProfile)

pytestmark = pytest.mark.gpu

COLS = ("node", "status", "score", "reservation", "gpu_minors", "rdma_minors")
COUNTERS = ("passes", "cut_passes", "rescans", "slot_misses", "bubble_passes")
Q_CPU, Q_MEM = synth.QDIM_CPU, synth.QDIM_MEMORY
KEYS_RAN = 2  # ks_stats.commit_helpers: the evaluator wave ran


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # must load the in-tree HIP library; no fallback
    return rt


def evaluator(runtime, cfg, nodes, quotas, keys, vshards=1):
    """a context of the dedicated kernel with the slot-key table (keys) or with the in-wave evaluation"""
    old = os.environ.get("KS_FQ_KEYS")
    os.environ["KS_FQ_KEYS"] = "1" if keys else "0"
    try:
        ev = runtime.Evaluator(cfg, nodes.copy(), quotas.copy())
    finally:
        if old is None:
            del os.environ["KS_FQ_KEYS"]
        else:
            os.environ["KS_FQ_KEYS"] = old
    if vshards > 1:
        ev.shard(1, 0, None, vshards)
    return ev


def three_way(runtime, oracle_lib, prof, nodes, quotas, queues, label, vshards=1, table_fits=True):
    """Schedules the queues one after the other on the oracle, the default path and the KS_FQ_KEYS=0 path; returns the
    oracle's results per queue and the default path's stats of the first queue."""
    cfg = prof.to_ks_config()
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas.copy(), nthreads=4)
    dflt = evaluator(runtime, cfg, nodes, quotas, True, vshards)
    wave0 = evaluator(runtime, cfg, nodes, quotas, False, vshards)
    wants, st0 = [], None
    try:
        for qi, pods in enumerate(queues):
            tag = f"{label} queue {qi}"
            want = orc.schedule(pods)
            got_k = dflt.schedule(pods)
            got_w = wave0.schedule(pods)
            s_k, s_w = dflt.stats(), wave0.stats()
            print(tag, {k: s_k[k] for k in COUNTERS}, "fast picks", s_k["diag"][7], "helpers", s_k["commit_helpers"],
                  s_w["commit_helpers"], "LDS", s_k["commit_lds_bytes"], s_w["commit_lds_bytes"])
            assert s_k["commit_helpers"] == (KEYS_RAN if table_fits else 0), f"{tag}: the default path's kernel variant"
            assert s_w["commit_helpers"] == 0, f"{tag}: KS_FQ_KEYS=0 still ran the evaluator wave"
            assert s_k["commit_lds_bytes"] <= 160 * 1024
            assert_same_results(got_k, want, f"{tag} keys/oracle")
            for k in COLS:
                assert np.array_equal(got_k[k], want[k]), f"{tag}: {k} differs from the oracle"
                assert np.array_equal(got_k[k], got_w[k]), f"{tag}: {k} differs between the two paths"
            assert_same_state(dflt.read_nodes(), orc.read_nodes(), f"{tag} keys/oracle")
            assert_same_state(dflt.read_nodes(), wave0.read_nodes(), f"{tag} keys/in-wave")
            assert np.array_equal(dflt.read_quota_used(), orc.read_quota_used()), f"{tag}: quota used differs from the oracle"
            assert np.array_equal(dflt.read_quota_used(), wave0.read_quota_used()), f"{tag}: quota used differs between paths"
            for k in COUNTERS:
                assert s_k[k] == s_w[k], f"{tag}: counter {k} {s_k[k]} != {s_w[k]}"
            assert s_k["diag"][7] == s_w["diag"][7], f"{tag}: fast picks differ"
            if st0 is None:
                st0 = s_k
            wants.append(want)
    finally:
        dflt.close()
        wave0.close()
        orc.close()
    return wants, st0


def flat_quotas(pods, n, rng, admit=0.9):
    return synth.make_quotas(pods, n, rng, admit_frac=admit)


@pytest.mark.parametrize("batch", [64, 7])
def test_passes_with_a_tail(runtime, oracle_lib, batch):
    """257 nodes, 130 pods: the last pass has 2 pods (passes of 64) or 4 (passes of 7), so the evaluator's lanes past
    the pass's pods must not store"""
    rng = np.random.Generator(np.random.PCG64(77))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = flat_quotas(pods, 4, rng, 0.7)
    wants, st = three_way(runtime, oracle_lib, profile(quota=True, check_parent=True, batch_pods=batch), nodes, q, [pods],
                          f"tail-b{batch}")
    assert st["passes"] >= (3 if batch == 64 else 19)
    stt = np.asarray(wants[0]["status"])
    assert (stt == abi.KS_S_SCHEDULED).any() and (stt & abi.KS_S_QUOTA).any()


def test_slot_reuse_and_unschedulable(runtime, oracle_lib):
    """40 nodes and 64 pods: most pods land on slots the pass already touched (a re-evaluation per Reserve); one pod in
    mid-pass fits no node and issues nothing"""
    rng = np.random.Generator(np.random.PCG64(9))
    nodes = synth.make_nodes(40, rng)
    pods = synth.make_pods(64, rng, 2)
    pods.req_milli_cpu[29] = 10 ** 9
    pods.nonzero_milli_cpu[29] = 10 ** 9
    pods.quota[29] = -1
    q = flat_quotas(pods, 2, rng, 2.0)
    wants, _ = three_way(runtime, oracle_lib, profile(quota=True), nodes, q, [pods], "reuse")
    stt = np.asarray(wants[0]["status"])
    assert stt[29] == abi.KS_S_UNSCHEDULABLE
    placed = np.asarray(wants[0]["node"])[stt == abi.KS_S_SCHEDULED]
    assert len(placed) > 40 >= len(np.unique(placed))


def test_candidate_pressure(runtime, oracle_lib):
    """candidates=2 with homogeneous pods: every pod's top is taken, so the run goes through the second-best rows, the
    misses (rows wave 0 builds itself), the rescans and cut passes (wave 0 leaves with evaluations pending)"""
    rng = np.random.Generator(np.random.PCG64(3))
    nodes = synth.make_nodes(257, rng)
    pods = homogeneous_pods(130)
    pods.quota[:] = np.arange(130) % 3
    pods.quota_req[Q_CPU] = pods.req_milli_cpu
    pods.quota_req[Q_MEM] = pods.req_memory
    pods.quota_mask[:] = (1 << Q_CPU) | (1 << Q_MEM)
    q = flat_quotas(pods, 3, rng, 0.95)
    _, st = three_way(runtime, oracle_lib, profile(quota=True, candidates=2), nodes, q, [pods], "pressure")
    assert st["cut_passes"] > 0
    assert st["rescans"] > 0
    assert st["slot_misses"] > 0


def divergent_workload(nsc):
    """40 nodes, 64 pods whose evaluation takes a different path per lane of the evaluator: PROD and non-PROD pods,
    DaemonSet pods, all-zero requests, a node with a capacity of 2^47 (>= 2^43: its terms take the int64 path for every
    pod) and a pod requesting 2^46 bytes (the int64 path on every node, and only that node fits it); nsc scalar slots"""
    rng = np.random.Generator(np.random.PCG64(1234 + nsc))
    nodes = synth.make_nodes(40, rng)
    pods = stress_pods(64, rng, 3)
    pods.flags[0::3] |= abi.KS_POD_PROD
    pods.flags[1::3] &= ~np.uint32(abi.KS_POD_PROD)
    pods.flags[5] |= abi.KS_POD_DAEMONSET
    nodes.alloc_memory[3] = 1 << 47
    nodes.la_alloc_memory[3] = 1 << 47
    pods.req_memory[10] = pods.nonzero_memory[10] = 1 << 46
    pods.quota[10] = -1
    if nsc == 0:
        nodes.alloc_scalar[:, :] = 0
        nodes.req_scalar[:, :] = 0
        pods.req_scalar[:, :] = 0
        pods.flags[:] &= ~np.uint32(abi.KS_POD_SCALAR_KEYS)
    if nsc == 4:
        # two more scalar slots, checked by the Filter: every third pod asks for some, a few nodes run short
        nodes.alloc_scalar[2] = 8
        nodes.alloc_scalar[3] = rng.integers(0, 4, 40)
        pods.req_scalar[2][::3] = 1
        pods.req_scalar[3][::4] = 1
        pods.flags[(pods.req_scalar[2] != 0) | (pods.req_scalar[3] != 0)] |= abi.KS_POD_SCALAR_KEYS
    return nodes, pods


@pytest.mark.parametrize("nsc", [0, 2, 4])
def test_per_lane_divergence(runtime, oracle_lib, nsc):
    nodes, pods = divergent_workload(nsc)
    res = {CPU: 1, MEMORY: 1, BATCH_CPU: 1, BATCH_MEMORY: 1} if nsc else {CPU: 1, MEMORY: 1}
    prof = SchedulerProfile(fit=NodeResourcesFitArgs(strategy="LeastAllocated", resources=res), fit_weight=1,
                            loadaware=LoadAwareSchedulingArgs(score_according_prod_usage=True), loadaware_weight=1,
                            quota=ElasticQuotaArgs(enable_check_parent_quota=False))
    rng = np.random.Generator(np.random.PCG64(8))
    q = flat_quotas(pods, 3, rng, 2.0)
    assert (pods.flags & abi.KS_POD_PROD).any() and not (pods.flags & abi.KS_POD_PROD).all()
    assert (pods.flags & abi.KS_POD_DAEMONSET).any()
    assert ((pods.req_milli_cpu == 0) & (pods.req_memory == 0)).any()
    wants, _ = three_way(runtime, oracle_lib, prof, nodes, q, [pods], f"divergence-nsc{nsc}")
    stt, node = np.asarray(wants[0]["status"]), np.asarray(wants[0]["node"])
    assert stt[10] == abi.KS_S_SCHEDULED and node[10] == 3, "the 2^46-byte pod belongs on the 2^47-byte node"
    placed = node[stt == abi.KS_S_SCHEDULED]
    assert len(placed) > len(np.unique(placed)), "no slot was reused"
    assert (placed[np.nonzero(stt == abi.KS_S_SCHEDULED)[0] > 10] == 3).any() or len(placed) > 40, \
        "no later pod was evaluated against the big node's slot"


def test_table_does_not_fit(runtime, oracle_lib):
    """candidates=64: the commit image has no room for the table, so the context keeps the in-wave evaluation"""
    rng = np.random.Generator(np.random.PCG64(21))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 4)
    q = flat_quotas(pods, 4, rng, 0.7)
    three_way(runtime, oracle_lib, profile(quota=True, candidates=64), nodes, q, [pods], "cand64", table_fits=False)


def test_two_virtual_shards(runtime, oracle_lib):
    rng = np.random.Generator(np.random.PCG64(41))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = flat_quotas(pods, 4, rng, 0.7)
    wants, _ = three_way(runtime, oracle_lib, profile(quota=True, check_parent=True), nodes, q, [pods], "vshards",
                         vshards=2)
    assert (np.asarray(wants[0]["status"]) & abi.KS_S_QUOTA).any()
