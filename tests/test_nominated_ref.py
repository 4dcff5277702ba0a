"""tests/nominated_ref.py -- the reference the GPU tests of the nominated-pod entry points compare against -- on
hand-worked cases that follow upstream's RunFilterPluginsWithNominatedPods / addNominatedPods step by step (kube-scheduler
v1.24 framework/runtime/framework.go, not on disk; the comments give the steps).  CPU only: the helper composes the
unchanged oracle.

Base case: node 0 with 4000m allocatable and 1000m requested (one pod), a nominated pod of 2000m at priority 10."""
import numpy as np

import nominated_ref as ref
import test_preempt as hand
from helpers import profile
from koordinator_amd import abi
from koordinator_amd.cluster import NominatedTable

GI = 1 << 30


def base(allowed=110):
    nodes = hand.cluster(1, alloc_cpu=4000, allowed=allowed)
    nodes.req_milli_cpu[0] = 1000
    nodes.req_memory[0] = GI
    nodes.pod_count[0] = 1
    return nodes


def entries(specs):
    """(node, priority, id, cpu); memory 1 GiB each"""
    t = NominatedTable(len(specs))
    for i, (node, prio, uid, cpu) in enumerate(specs):
        t.node[i], t.priority[i], t.id[i] = node, prio, uid
        t.req[0, i], t.req[1, i] = cpu, GI
    return t


def pod(cpu=1500):
    p = hand.preemptor(cpu)
    p.quota[0] = -1  # (no ElasticQuota in this profile)
    p.quota_mask[0] = 0
    return p


def run(oracle_lib, nodes, nom, prio, **kw):
    return ref.evaluate(oracle_lib, profile().to_ks_config(), nodes, {}, nom, pod(), prio, **kw)


def test_lower_priority_pod_sees_the_nominated_pod(oracle_lib):
    # priority 5 < 10: the entry counts.  Pass 1: Requested 1000 + 2000 = 3000, 1500 > 4000 - 3000 -> Insufficient cpu;
    # pass 1 failed, so its status is the node's
    w = run(oracle_lib, base(), entries([(0, 10, 7, 2000)]), 5)
    assert w["reasons"][0] == abi.KS_R_FIT_CPU
    assert w["pass2"][0] == 0  # without the nominated pod the node has room: this is the room it keeps
    assert w["total"][0] == -1 and not w["scores"][0].any()


def test_higher_priority_pod_does_not(oracle_lib):
    # priority 20 > 10: no entry counts, the Filters run once on Requested 1000: 1500 <= 3000
    w = run(oracle_lib, base(), entries([(0, 10, 7, 2000)]), 20)
    assert w["reasons"][0] == 0 and w["total"][0] >= 0


def test_own_entry_is_skipped(oracle_lib):
    # priority 10 >= 10 would count, but the entry is the pod's own (UID == UID(P)): feasible
    nom = entries([(0, 10, 7, 2000)])
    assert run(oracle_lib, base(), nom, 10, self_id=7)["reasons"][0] == 0
    # the same priority under another id: the entry counts (>=, not >)
    assert run(oracle_lib, base(), nom, 10, self_id=8)["reasons"][0] == abi.KS_R_FIT_CPU


def test_pod_count_limit_reached_by_a_nominated_pod(oracle_lib):
    # 2 pods allowed, 1 running: alone the pod fits (1 + 1 <= 2); with the nominated pod added the node holds 2 and
    # 2 + 1 > 2 -> Too many pods (its 100m leave the cpu check passing: 1500 <= 4000 - 1100)
    w = run(oracle_lib, base(allowed=2), entries([(0, 10, 7, 100)]), 5)
    assert w["reasons"][0] == abi.KS_R_FIT_PODS and w["pass2"][0] == 0


def test_only_the_entries_at_or_above_the_priority_count(oracle_lib):
    # entries of 1000m at priority 10 and 2000m at priority 3, pod at priority 5: only the first counts.
    # Requested 1000 + 1000 = 2000: 1500 <= 2000 -> pass 1 passes, pass 2 passes: feasible.  Were both counted
    # (Requested 4000) the pod would not fit; a pod at priority 3 sees both.
    nom = entries([(0, 10, 7, 1000), (0, 3, 8, 2000)])
    assert run(oracle_lib, base(), nom, 5)["reasons"][0] == 0
    assert run(oracle_lib, base(), nom, 3)["reasons"][0] == abi.KS_R_FIT_CPU
    req, cnt = nom.sums(1, 5)
    assert req[0, 0] == 1000 and cnt[0] == 1


def test_scores_are_over_the_remaining_feasible_set(oracle_lib):
    # two nodes; the nominated pod takes node 0's room for a priority-5 pod, so node 1 is the winner and the summary
    # counts node 0 under Insufficient cpu
    nodes = hand.cluster(2, alloc_cpu=4000)
    nodes.req_milli_cpu[:] = [1000, 2000]
    nodes.nonzero_milli_cpu[:] = nodes.req_milli_cpu  # (Fit scores on NonZeroRequested)
    nodes.req_memory[:] = GI
    nodes.pod_count[:] = 1
    w = ref.evaluate(oracle_lib, profile().to_ks_config(), nodes, {}, entries([(0, 10, 7, 2000)]), pod(), 5)
    assert list(w["reasons"]) == [abi.KS_R_FIT_CPU, 0]
    s = ref.summary(w, 2, abi.KS_R_FIT_CPU)
    assert s["feasible"] == 1 and s["best_node"] == 1 and list(s["top_nodes"]) == [1]
    assert s["reason_nodes"][abi.KS_R_FIT_CPU.bit_length() - 1] == 1 and s["unresolvable"] == 1
    # evaluateNominatedNode: a priority-20 pod nominated to node 1 gets node 1 alone although node 0 scores higher
    w = ref.evaluate(oracle_lib, profile().to_ks_config(), nodes, {}, entries([(0, 10, 7, 2000)]), pod(), 20,
                     nominated_node=1)
    assert list(w["reasons"]) == [0, 0] and w["total"][0] > w["total"][1] and w["single"] == 1
    s = ref.summary(w, 2, 0)
    assert s["feasible"] == 1 and s["best_node"] == 1 and s["best_total"] == w["total"][1]
