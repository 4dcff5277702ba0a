"""The dedicated Fit + LoadAware + ElasticQuota commit kernel (ks_fq.h) against the CPU oracle and against the general
commit kernel (KS_COMMIT_FQ=0, read when a context is created): every result column, the node state, the quota `used`
table and the pass counters.  `npused` has no read-back entry point, so a second queue of non-preemptible pods is
scheduled on the same contexts: its admissions against `min` depend on the `npused` the first queue left.

The shapes are the smallest at which the kernel can still go wrong: 257 nodes (5 chunks, the last with one node),
130 pods (three passes, the last with 2 pods), passes of 64 and of 7 pods.
"""
import os

import numpy as np
import pytest

from helpers import assert_same_results, assert_same_state, homogeneous_pods, profile
from koordinator_amd import abi, synth
from koordinator_amd.cluster import QuotaTable

pytestmark = pytest.mark.gpu

COLS = ("node", "status", "score", "reservation", "gpu_minors", "rdma_minors")
COUNTERS = ("passes", "cut_passes", "rescans", "slot_misses", "bubble_passes")
Q_CPU, Q_MEM = synth.QDIM_CPU, synth.QDIM_MEMORY


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # must load the in-tree HIP library; no fallback
    return rt


def evaluator(runtime, cfg, nodes, quotas, fq, vshards=1):
    """a context on the dedicated kernel (fq) or on the general one"""
    old = os.environ.get("KS_COMMIT_FQ")
    os.environ["KS_COMMIT_FQ"] = "1" if fq else "0"
    try:
        ev = runtime.Evaluator(cfg, nodes.copy(), quotas.copy())
    finally:
        if old is None:
            del os.environ["KS_COMMIT_FQ"]
        else:
            os.environ["KS_COMMIT_FQ"] = old
    if vshards > 1:
        ev.shard(1, 0, None, vshards)
    return ev


def three_way(runtime, oracle_lib, prof, nodes, quotas, queues, label, vshards=1):
    """Schedules the queues one after the other on the oracle, the dedicated kernel and the general kernel; returns
    the oracle's results per queue and the dedicated kernel's stats of the first queue."""
    cfg = prof.to_ks_config()
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas.copy(), nthreads=4)
    fq = evaluator(runtime, cfg, nodes, quotas, True, vshards)
    gen = evaluator(runtime, cfg, nodes, quotas, False, vshards)
    wants, st0 = [], None
    try:
        for qi, pods in enumerate(queues):
            tag = f"{label} queue {qi}"
            want = orc.schedule(pods)
            got_fq = fq.schedule(pods)
            got_gen = gen.schedule(pods)
            assert_same_results(got_fq, want, f"{tag} fq/oracle")
            for k in COLS:
                assert np.array_equal(got_fq[k], got_gen[k]), f"{tag}: {k} differs between the two kernels"
                assert np.array_equal(got_fq[k], want[k]), f"{tag}: {k} differs from the oracle"
            assert_same_state(fq.read_nodes(), orc.read_nodes(), f"{tag} fq/oracle")
            assert_same_state(fq.read_nodes(), gen.read_nodes(), f"{tag} fq/general")
            assert np.array_equal(fq.read_quota_used(), orc.read_quota_used()), f"{tag}: quota used differs from the oracle"
            assert np.array_equal(fq.read_quota_used(), gen.read_quota_used()), f"{tag}: quota used differs between kernels"
            s_fq, s_gen = fq.stats(), gen.stats()
            for k in COUNTERS:
                assert s_fq[k] == s_gen[k], f"{tag}: counter {k} {s_fq[k]} != {s_gen[k]}"
            assert s_fq["diag"][7] == s_gen["diag"][7], f"{tag}: fast picks differ"
            if st0 is None:
                st0 = s_fq
            wants.append(want)
    finally:
        fq.close()
        gen.close()
        orc.close()
    return wants, st0


def np_followup(pods, n=40):
    """non-preemptible copies of the first pods: admitted against `min` by the npused the queue before left"""
    t = synth.make_pods(n, np.random.Generator(np.random.PCG64(5)), 1)
    t.quota[:] = pods.quota[:n]
    t.flags[:] |= abi.KS_POD_NONPREEMPTIBLE
    return t


def edge_workload():
    """257 nodes, 130 pods, 7 quota rows: leaves 0, 1 under 4 under 5 (a three-level chain whose top limit is the
    tight one), leaf 2 at its limit, leaf 3 with a tight min, leaf 6 generous; rows 4, 5 hold no pods."""
    rng = np.random.Generator(np.random.PCG64(77))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 1)
    n = pods.n
    pods.quota[:] = np.array([0, 1, 2, 3, 6, 2, 0, 3])[np.arange(n) % 8]
    pods.quota[::17] = -1  # pods without a quota
    pods.flags[(pods.quota == 3) & (np.arange(n) % 16 < 8)] |= abi.KS_POD_NONPREEMPTIBLE
    # a request in a dimension no quota limits
    odd = np.arange(n) % 5 == 0
    pods.quota_mask[odd] |= np.uint32(1 << 5)
    pods.quota_req[5][odd] = 1 << 50
    q = QuotaTable(7)
    mask = (1 << Q_CPU) | (1 << Q_MEM) | (1 << synth.QDIM_BATCH_CPU) | (1 << synth.QDIM_BATCH_MEMORY)
    q.limit_mask[:] = mask
    q.limit[:, :] = 1 << 45
    q.parent[:] = -1
    q.parent[0] = q.parent[1] = 4
    q.parent[4] = 5
    dem = lambda rows, d, upto: int(pods.quota_req[d][:upto][np.isin(pods.quota[:upto], rows)].sum())
    q.limit[Q_CPU][5] = dem([0, 1], Q_CPU, 40)   # the chain's top: full inside the first pass
    q.limit[Q_CPU][2] = dem([2], Q_CPU, 30) + 300  # leaf 2: full inside the first pass, small pods still fit
    q.min_mask[3] = mask
    q.min[:, 3] = 1 << 45
    q.min[Q_CPU][3] = 6000
    return nodes, pods, q


def assert_edges(want, pods):
    """every admission case is present in the oracle's output"""
    st, qt = np.asarray(want["status"]), pods.quota
    ok = st == abi.KS_S_SCHEDULED
    assert (ok & (qt < 0)).any(), "no pod without a quota was placed"
    leaf = np.nonzero(qt == 2)[0]
    rej = [i for i in leaf if st[i] == abi.KS_S_QUOTA]
    assert rej, "leaf 2 rejected nothing"
    assert any(ok[k] and k > i and k // 64 == i // 64 for i in rej for k in leaf), \
        "no smaller pod of the full leaf was admitted later in the same pass"
    assert (st == abi.KS_S_QUOTA_NONPREEMPTIBLE).any(), "no non-preemptible pod was rejected against min"
    assert (st[np.isin(qt, [0, 1])] == (abi.KS_S_QUOTA | abi.KS_S_QUOTA_PARENT)).any(), "no ancestor limit rejected"
    assert (ok & (pods.quota_req[5] > (1 << 45)) & (qt >= 0)).any(), "no pod with an unlimited dimension was placed"


@pytest.mark.parametrize("batch", [64, 7])
def test_quota_edges(runtime, oracle_lib, batch):
    nodes, pods, q = edge_workload()
    prof = profile(quota=True, check_parent=True, batch_pods=batch)
    wants, st = three_way(runtime, oracle_lib, prof, nodes, q, [pods, np_followup(pods)], f"edges-b{batch}")
    assert_edges(wants[0], pods)
    assert st["passes"] >= (3 if batch == 64 else 19)
    s1 = np.asarray(wants[1]["status"])
    assert (s1 == abi.KS_S_QUOTA_NONPREEMPTIBLE).any() and (s1 == abi.KS_S_SCHEDULED).any(), \
        "the follow-up queue does not depend on npused"


def test_quota_edges_leaf_only(runtime, oracle_lib):
    """the same tree without the ancestor check: the usage update still walks up the chain"""
    nodes, pods, q = edge_workload()
    wants, _ = three_way(runtime, oracle_lib, profile(quota=True, prod_usage=True), nodes, q, [pods, np_followup(pods)],
                         "edges-leaf")
    assert not (np.asarray(wants[0]["status"]) & abi.KS_S_QUOTA_PARENT).any()


def flat_quotas(pods, n, rng, admit=0.9):
    return synth.make_quotas(pods, n, rng, admit_frac=admit)


def test_candidate_pressure(runtime, oracle_lib):
    """candidates=2 with homogeneous pods: every pod's top is taken, so the run goes through the second-best rows, the
    rescans, cut passes and the touched-slot evaluation"""
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


def test_slot_reuse_and_unschedulable(runtime, oracle_lib):
    """40 nodes and 64 pods: most pods land on slots the pass already touched; one pod in mid-pass fits no node"""
    rng = np.random.Generator(np.random.PCG64(9))
    nodes = synth.make_nodes(40, rng)
    pods = synth.make_pods(64, rng, 2)
    pods.req_milli_cpu[29] = 10 ** 9
    pods.nonzero_milli_cpu[29] = 10 ** 9
    pods.quota[29] = -1
    q = flat_quotas(pods, 2, rng, 2.0)
    wants, st = three_way(runtime, oracle_lib, profile(quota=True), nodes, q, [pods], "reuse")
    stt = np.asarray(wants[0]["status"])
    assert stt[29] == abi.KS_S_UNSCHEDULABLE
    placed = np.asarray(wants[0]["node"])[stt == abi.KS_S_SCHEDULED]
    assert len(placed) > 40 >= len(np.unique(placed))


def test_non_monotone_profile_keeps_the_general_kernel(runtime, oracle_lib):
    """MostAllocated Fit with quotas is not this kernel's plugin set: the switch changes nothing"""
    rng = np.random.Generator(np.random.PCG64(21))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 4)
    q = flat_quotas(pods, 4, rng, 0.7)
    three_way(runtime, oracle_lib, profile(strategy="MostAllocated", quota=True, candidates=4), nodes, q, [pods], "most")


def test_two_virtual_shards(runtime, oracle_lib):
    rng = np.random.Generator(np.random.PCG64(41))
    nodes = synth.make_nodes(257, rng)
    pods = synth.make_pods(130, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = flat_quotas(pods, 4, rng, 0.7)
    wants, _ = three_way(runtime, oracle_lib, profile(quota=True, check_parent=True), nodes, q, [pods], "vshards",
                         vshards=2)
    assert (np.asarray(wants[0]["status"]) & abi.KS_S_QUOTA).any()
