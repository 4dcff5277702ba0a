"""Pins tests/nominated_queue_ref.py (the composed reference of ks_schedule_nominated) on hand-worked two-node cases,
and checks on the CPU that the workload tests/test_gpu_nominated_queue.py runs is not vacuous."""
import numpy as np
import pytest

import nominated_queue_ref as qref
from koordinator_amd import abi, synth
from koordinator_amd.cluster import NominatedTable


def two_nodes(oracle_lib, n_pods=2):
    """C2 on two nodes that pass LoadAware's Filter: node 0 half full, node 1 nearly empty (every plugin prefers
    node 1); small preemptible pods whose quota admits them"""
    w = synth.c2(n_nodes=16, n_pods=n_pods)
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ok = np.flatnonzero((orc.eval_pod(w.pods.rows([0]))[0] & ~np.uint32(qref.FIT_BITS)) == 0)
    finally:
        orc.close()
    w.nodes = w.nodes.rows(ok[:2])
    nd = w.nodes
    for i, div in ((0, 2), (1, 16)):
        nd.req_milli_cpu[i] = nd.nonzero_milli_cpu[i] = nd.alloc_milli_cpu[i] // div
        nd.req_memory[i] = nd.nonzero_memory[i] = nd.alloc_memory[i] // div
        nd.pod_count[i] = 10
    w.pods.flags[:] = abi.KS_POD_PROD
    w.pods.req_milli_cpu[:] = w.pods.nonzero_milli_cpu[:] = w.pods.la_req_cpu[:] = 1000
    w.pods.req_memory[:] = w.pods.nonzero_memory[:] = w.pods.la_req_memory[:] = 1 << 30
    w.pods.quota_req[:] = 0
    return w


def one_row(node, prio, rid, cpu):
    t = NominatedTable(1)
    t.node[0], t.priority[0], t.id[0], t.req[0, 0] = node, prio, rid, cpu
    return t


def run(oracle_lib, w, nom, prio, nn=None, sid=None):
    return qref.schedule(oracle_lib, w.cfg, w.nodes, w.quotas, nom, w.pods, prio, nn, sid)


def baseline(oracle_lib, w):
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        return orc.schedule(w.pods)
    finally:
        orc.close()


def test_both_pods_are_kept_off_the_room_of_a_higher_priority_nomination(oracle_lib):
    w = two_nodes(oracle_lib)
    assert list(baseline(oracle_lib, w)["node"]) == [1, 1]  # the premise: node 1 wins without a table
    room = int(w.nodes.alloc_milli_cpu[1] - w.nodes.req_milli_cpu[1])
    got = run(oracle_lib, w, one_row(1, 1000, 7, room - 500), [500, 500])
    assert list(got["status"]) == [0, 0] and list(got["node"]) == [0, 0]  # 1000 m do not fit into the 500 m left
    assert got["live"].m == 1
    # a pod above the row's priority does not count it
    got = run(oracle_lib, w, one_row(1, 1000, 7, room - 500), [500, 1001])
    assert list(got["node"]) == [0, 1]


def test_an_owner_takes_its_node_although_the_other_scores_higher(oracle_lib):
    w = two_nodes(oracle_lib)
    assert list(baseline(oracle_lib, w)["node"]) == [1, 1]
    got = run(oracle_lib, w, one_row(0, 1000, 7, 1000), [1000, 500], nn=[0, -1], sid=[7, -1])
    assert list(got["status"]) == [0, 0] and list(got["node"]) == [0, 1]
    assert got["live"].m == 0  # retired on Reserve


def test_an_owner_whose_node_fails_lands_elsewhere_and_its_row_is_retired(oracle_lib):
    w = two_nodes(oracle_lib)
    w.nodes.allowed_pods[0] = w.nodes.pod_count[0]  # node 0 takes no pod
    room0 = int(w.nodes.alloc_milli_cpu[0] - w.nodes.req_milli_cpu[0])
    got = run(oracle_lib, w, one_row(0, 1000, 7, room0), [1000, 500], nn=[0, -1], sid=[7, -1])
    assert list(got["status"]) == [0, 0] and list(got["node"]) == [1, 1]
    assert got["live"].m == 0


def test_a_quota_rejected_owner_keeps_its_row(oracle_lib):
    w = two_nodes(oracle_lib)
    assert w.pods.quota[0] >= 0
    w.pods.quota_req[synth.QDIM_CPU, 0] = 1 << 40
    room = int(w.nodes.alloc_milli_cpu[1] - w.nodes.req_milli_cpu[1])
    got = run(oracle_lib, w, one_row(1, 1000, 7, room - 500), [1000, 500], nn=[1, -1], sid=[7, -1])
    assert got["status"][0] in (abi.KS_S_QUOTA, abi.KS_S_QUOTA_PARENT) and got["node"][0] == -1
    assert got["live"].m == 1 and got["live"].id[0] == 7
    assert got["status"][1] == 0 and got["node"][1] == 0  # the row still keeps the second pod off node 1


@pytest.mark.parametrize("static", [False, True], ids=["c2", "c2-taint-affinity"])
def test_the_gpu_workload_is_not_vacuous(oracle_lib, static):
    w, nom, prio, nn, sid = qref.workload(static)
    assert 85 <= nom.m <= 95 and (nom.node == qref.WIDE).sum() == 70 and len(np.unique(nom.node)) == 10
    got = qref.schedule(oracle_lib, w.cfg, w.nodes, w.quotas, nom, w.pods, prio, nn, sid, trace=True)
    base = baseline(oracle_lib, w)
    tr = got["trace"]
    owners = set(qref.OWNER_POS)
    assert (got["node"] != base["node"]).sum() >= 5
    assert any(t["below_best_other"] for i, t in enumerate(tr) if i in owners)
    assert any(t["on_live_row_node"] for i, t in enumerate(tr) if i not in owners and i % 64 != 63)
    assert any(t["flip"] for t in tr)
    # the owners of the issue's list: the full nominated node sends its owner elsewhere, the quota rejects one
    f = qref.FULL_OWNER
    assert got["status"][f] == 0 and got["node"][f] != nn[f] and tr[f]["single"] == -1
    assert got["status"][qref.QUOTA_OWNER] in (abi.KS_S_QUOTA, abi.KS_S_QUOTA_PARENT)
    assert (np.diff(sorted(qref.OWNER_POS)) == 1).any() and {0, 63, 64} <= owners
    assert sum(int(got["status"][i] == 0) for i in owners) >= 5
    assert got["live"].m == nom.m - sum(int(got["status"][i] == 0) for i in owners)


def test_the_rescan_workload_puts_a_closed_nominated_node_among_a_rescanned_chunk(oracle_lib):
    """the premises of tests/test_gpu_nominated_queue.py::test_rescan_applies_the_table: without a table the nominated
    node is the best node for the pods; with it the first two pods take the chunk's two best open nodes, so for every
    later pod the chunk's best and runner-up are both touched and their current keys lie below the runner-up's swept
    key; some later pod goes to a node that was neither (found only by re-scanning the chunk's untouched nodes), and no
    pod ever lands on the nominated node"""
    w, nom, prio = qref.rescan_workload(oracle_lib)
    base = baseline(oracle_lib, w)
    assert base["node"][0] == qref.RESCAN_NOM
    got = run(oracle_lib, w, nom, prio)
    assert (got["status"] == 0).all()
    assert sorted(got["node"][:2]) == [qref.RESCAN_A, qref.RESCAN_B]
    assert (got["score"][2:] < got["score"][1]).all()
    assert (~np.isin(got["node"][2:], (qref.RESCAN_A, qref.RESCAN_B))).any()
    assert not (got["node"] == qref.RESCAN_NOM).any() and got["live"].m == 1
