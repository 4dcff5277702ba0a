"""The expected result of an evaluation with nominated pods, composed from the unchanged CPU oracle.

kube-scheduler v1.24 (framework/runtime/framework.go RunFilterPluginsWithNominatedPods + addNominatedPods,
schedule_one.go evaluateNominatedNode; restated, upstream is not on disk):

  1. For pod P on node X the nominated pods that count are those nominated to X with priority >= priority(P) and
     UID != UID(P).  None: the Filters run once.  Otherwise pass 1 runs on a NodeInfo copy with them added (Requested,
     every scalar and the pod count go up); if it fails, its status is the node's; if it passes, pass 2 runs without
     them and its status is the node's.
  2. Scores are computed without the nominated pods, over the nodes rule 1 leaves feasible.
  4. If P itself has a nominated node and that node passes rule 1, it is the only feasible node.

Nothing here restates a plugin: pass 1 is the oracle on a node table with the counted sums added, pass 2 the oracle on
the table as it is, and the scores come from the oracle on the table in which every node that rule 1 (or rule 4) takes
out of the feasible set has its allocatable pod count set to 0, which removes exactly those nodes and changes nothing
about the others.
"""
from __future__ import annotations

import numpy as np

from koordinator_amd import abi


def with_nominated(nodes, nom, priority: int, self_id: int = -1):
    """a copy of the node table with the nominated pods that count for (priority, self_id) added (AddPodInfo)"""
    req, cnt = nom.sums(nodes.n, priority, self_id)
    t = nodes.copy()
    t.req_milli_cpu[:] = t.req_milli_cpu + req[0]
    t.req_memory[:] = t.req_memory + req[1]
    t.req_ephemeral[:] = t.req_ephemeral + req[2]
    for k in range(abi.KS_MAX_SCALARS):
        t.req_scalar[k] = t.req_scalar[k] + req[3 + k]
    t.pod_count[:] = t.pod_count + cnt
    return t, cnt


def _eval(oracle_lib, cfg, nodes, tables, pod):
    orc = oracle_lib.Oracle(cfg, nodes, **{k: v.copy() for k, v in tables.items()})
    try:
        return orc.eval_pod(pod)
    finally:
        orc.close()


def evaluate(oracle_lib, cfg, nodes, tables, nom, pod, priority: int, nominated_node: int = -1, self_id: int = -1):
    """{reasons, scores, total}: every node's status under rule 1 and the scores of rule 2; `single` is the pod's
    nominated node when rule 4 makes it the only feasible node (else -1), and single_scores / single_total its row
    normalized over that one-node set."""
    added, cnt = with_nominated(nodes, nom, priority, self_id)
    r1 = _eval(oracle_lib, cfg, added, tables, pod)[0]
    r2 = _eval(oracle_lib, cfg, nodes.copy(), tables, pod)[0]
    reasons = np.where((cnt > 0) & (r1 != 0), r1, r2).astype(np.uint32)
    excluded = (reasons != 0) & (r2 == 0)  # fails only with the nominated pods added
    cut = nodes.copy()
    cut.allowed_pods[excluded] = 0
    r3, scores, total = _eval(oracle_lib, cfg, cut, tables, pod)
    keep = ~excluded
    assert np.array_equal(r3[keep], r2[keep]), "emptying the excluded nodes changed another node's status"
    assert (total[excluded] == -1).all() and not scores[excluded].any()
    out = {"reasons": reasons, "scores": scores, "total": total, "single": -1, "pass1": r1, "pass2": r2}
    if nominated_node >= 0 and reasons[nominated_node] == 0:
        one = nodes.copy()
        others = np.arange(nodes.n) != nominated_node
        one.allowed_pods[others] = 0
        r4, s4, t4 = _eval(oracle_lib, cfg, one, tables, pod)
        assert r4[nominated_node] == 0 and (r4[others] != 0).all()
        out.update(single=int(nominated_node), single_scores=s4[nominated_node], single_total=int(t4[nominated_node]))
    return out


def summary(want: dict, top_n: int, mask: int) -> dict:
    """ks_pod_summary of an evaluate() result: the reason counts and the unresolvable set are every node's own status;
    the feasible set, the winner and the top rows are the one node when rule 4 applies"""
    reasons = want["reasons"]
    n = len(reasons)
    scores, total = want["scores"], want["total"]
    feas = reasons == 0
    if want["single"] >= 0:
        feas = np.zeros(n, bool)
        feas[want["single"]] = True
        scores, total = scores.copy(), total.copy()
        scores[want["single"]] = want["single_scores"]
        total[want["single"]] = want["single_total"]
    idx = np.flatnonzero(feas)
    order = idx[np.lexsort((idx, -np.asarray(total, np.int64)[idx]))]
    top = order[:top_n]
    unres = (reasons & np.uint32(mask)) != 0
    return {
        "nodes": n, "feasible": int(feas.sum()), "unresolvable": int(unres.sum()),
        "reason_nodes": np.array([int(((reasons >> np.uint32(b)) & np.uint32(1)).sum()) for b in range(32)], np.int64),
        "best_node": int(order[0]) if len(order) else -1,
        "best_total": int(total[order[0]]) if len(order) else -1,
        "top_nodes": top.astype(np.int32), "top_totals": np.asarray(total, np.int64)[top],
        "top_scores": np.asarray(scores, np.int64)[top], "feasible_mask": feas, "unresolvable_mask": unres,
    }


def preempt(oracle_lib, cfg, nodes, quotas, node_pods, nom, pod, priority: int, self_id: int = -1, **kw) -> dict:
    """Oracle.preempt on the table with Requested and pod count plus the sums for the preemptor's priority (its own
    entry excluded): every Fit check of every dry run then sees them, the quota checks do not"""
    added, _ = with_nominated(nodes, nom, priority, self_id)
    orc = oracle_lib.Oracle(cfg, added, quotas.copy())
    try:
        orc.load_node_pods(node_pods)
        return orc.preempt(pod, priority, node_status=True, **kw)
    finally:
        orc.close()
