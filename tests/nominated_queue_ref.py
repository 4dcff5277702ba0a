"""The expected result of the batched queue with a nominated table loaded (ks_schedule_nominated), composed from the
unchanged CPU oracle like tests/nominated_ref.py.  Nothing here restates a plugin.

One persistent Oracle holds the state.  For every pod in queue order:

  1. the current node and quota tables are read from it (read_nodes + read_quota_used);
  2. nominated_ref.evaluate runs with the live rows (rules 1, 2 and 4 of that module);
  3. every node rule 1 excludes gets allowed_pods = 0 -- or, when the pod's own nominated node is feasible, every
     other node does;
  4. a fresh Oracle schedules that one pod on the table of step 3: status, node and score with the ElasticQuota
     admission and the lowest-index tie-break;
  5. a scheduled pod is assumed on the persistent oracle and its own row leaves the live table (upstream assume ->
     DeleteNominatedPodIfExists); an unschedulable or quota-rejected pod keeps its row.

The quota table handed to the fresh oracle carries `used` only (there is no read-back of the non-preemptible usage),
so the queue's pods must be preemptible; schedule() asserts it.

workload() builds the case tests/test_gpu_nominated_queue.py runs and tests/test_nominated_queue_ref.py checks for
non-vacuity on the CPU.
"""
from __future__ import annotations

import numpy as np

import nominated_ref as ref
from koordinator_amd import abi, synth
from koordinator_amd.cluster import NominatedTable

N_NODES, N_PODS = 200, 192
WIDE = 17                                   # the node with 70 rows
OWNER_POS = (0, 63, 64, 100, 101, 130, 150, 170)
FULL_OWNER, QUOTA_OWNER = 130, 150          # the owner whose nominated node is full, the one its quota rejects
PRIOS = (500, 1000, 1500)
FIT_BITS = (abi.KS_R_FIT_PODS | abi.KS_R_FIT_CPU | abi.KS_R_FIT_MEMORY | abi.KS_R_FIT_EPHEMERAL | abi.KS_R_FIT_SCALAR)


def current(nodes, quotas, orc):
    """the node and quota tables as the oracle holds them after its assumes"""
    st = orc.read_nodes().as_dict()
    t = nodes.copy()
    for k, v in st.items():
        if k not in ("host_ports", "topo_count"):
            getattr(t, k)[...] = v
    q = quotas.copy()
    q.used[:] = orc.read_quota_used().T
    return t, q


def _one(oracle_lib, cfg, nodes, quotas, pod):
    orc = oracle_lib.Oracle(cfg, nodes, quotas=quotas)
    try:
        return orc.schedule(pod)
    finally:
        orc.close()


def schedule(oracle_lib, cfg, nodes, quotas, nom, pods, priority, nominated_node=None, self_id=None, trace=False):
    """{status, node, score} of the queue, the persistent oracle's final {nodes, quota_used}, the surviving table
    `live`, and with trace=True per pod what the non-vacuity conditions need"""
    p = pods.n
    priority = np.asarray(priority, np.int64)
    nominated_node = np.full(p, -1, np.int64) if nominated_node is None else np.asarray(nominated_node, np.int64)
    self_id = np.full(p, -1, np.int64) if self_id is None else np.asarray(self_id, np.int64)
    assert not (pods.flags & abi.KS_POD_NONPREEMPTIBLE).any(), "the composed reference carries quota `used` only"
    out = {k: np.zeros(p, dt) for k, dt in (("status", np.uint32), ("node", np.int32), ("score", np.int64))}
    live = nom.copy()
    retired = nom.rows([])
    tr = []
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas=quotas.copy())
    try:
        for i in range(p):
            cur, q = current(nodes, quotas, orc)
            pod = pods.rows([i])
            who = dict(priority=int(priority[i]), nominated_node=int(nominated_node[i]), self_id=int(self_id[i]))
            want = ref.evaluate(oracle_lib, cfg, cur, {"quotas": q}, live, pod, **who)
            cut = cur.copy()
            if want["single"] >= 0:
                cut.allowed_pods[np.arange(cur.n) != want["single"]] = 0
            else:
                cut.allowed_pods[(want["reasons"] != 0) & (want["pass2"] == 0)] = 0
            r = _one(oracle_lib, cfg, cut, q.copy(), pod)
            for k in out:
                out[k][i] = r[k][0]
            if trace:
                t = {"single": want["single"], "on_live_row_node": False, "below_best_other": False, "flip": False}
                if r["status"][0] == abi.KS_S_SCHEDULED:
                    t["on_live_row_node"] = bool((live.node == r["node"][0]).any())
                if want["single"] >= 0:
                    others = (want["reasons"] == 0) & (np.arange(cur.n) != want["single"])
                    t["below_best_other"] = bool(others.any() and want["single_total"] < want["total"][others].max())
                if retired.m:
                    both = concat(live, retired)
                    w2 = ref.evaluate(oracle_lib, cfg, cur, {"quotas": q}, both, pod, **who)
                    rn = np.unique(retired.node)
                    t["flip"] = bool(((w2["reasons"][rn] != 0) & (want["reasons"][rn] == 0)).any())
                tr.append(t)
            if r["status"][0] == abi.KS_S_SCHEDULED:
                orc.assume(pod, int(r["node"][0]))
                if self_id[i] >= 0:
                    retired = concat(retired, live.rows(np.flatnonzero(live.id == self_id[i])))
                    live = live.rows(np.flatnonzero(live.id != self_id[i]))
        out["nodes"] = orc.read_nodes().as_dict()
        out["quota_used"] = orc.read_quota_used()
    finally:
        orc.close()
    out["live"] = live
    out["trace"] = tr
    return out


def concat(a, b):
    t = NominatedTable(a.m + b.m)
    for k in ("node", "priority", "id"):
        getattr(t, k)[:] = np.concatenate([getattr(a, k), getattr(b, k)])
    t.req[:, : a.m] = a.req
    t.req[:, a.m:] = b.req
    return t


def room(nodes, i):
    return int(nodes.alloc_milli_cpu[i] - nodes.req_milli_cpu[i])


def workload(static: bool, seed: int = 7):
    """(w, nom, priority, nominated_node, self_id): C2 (static: with BalancedAllocation, TaintToleration, NodeAffinity)
    on 200 nodes, 192 pods = three 64-pod windows; ~90 rows on 10 nodes, 70 of them on WIDE, the others 1-4 rows of
    mixed priority; 8 owner pods at OWNER_POS (the queue's first pod, both sides of a window boundary, two adjacent
    ones, one whose nominated node is full, one its quota rejects)."""
    w = (synth.c2_default if static else synth.c2)(n_nodes=N_NODES, n_pods=N_PODS)
    if static:
        w.profile.node_ports = False
    rng = np.random.default_rng(seed)
    w.pods.flags[:] = w.pods.flags & ~np.uint32(abi.KS_POD_NONPREEMPTIBLE)
    nodes = w.nodes
    # the nominated nodes: WIDE, then nine more spread over the chunks; they are the emptiest nodes of the cluster, so
    # the pods the table does not keep off go there first
    others = [0, 63, 64, 65, 127, 128, 150, 190, 199]
    for i in [WIDE] + others:
        nodes.req_milli_cpu[i] = nodes.nonzero_milli_cpu[i] = nodes.alloc_milli_cpu[i] // 8
        nodes.req_memory[i] = nodes.nonzero_memory[i] = nodes.alloc_memory[i] // 8
    rows = [(WIDE, PRIOS[j % 3], 200 + j, 250 + j, 64 << 20) for j in range(70)]
    uid = 0
    owner_rows = []
    for k, i in enumerate(others):
        cnt = 1 + k % 4
        for j in range(cnt):
            prio = PRIOS[(k + j) % 3] + 1
            # the first row of a node takes most of its room (it is an owner's), the others a sliver
            cpu = room(nodes, i) * 3 // 4 if j == 0 else 100
            rows.append((i, prio, uid, cpu, 256 << 20))
            if j == 0:
                owner_rows.append((i, prio, uid))
            uid += 1
    nom = NominatedTable(len(rows))
    for r, (node, prio, rid, cpu, mem) in enumerate(rows):
        nom.node[r], nom.priority[r], nom.id[r] = node, prio, rid
        nom.req[0, r], nom.req[1, r] = cpu, mem
    p = w.pods.n
    priority = rng.choice(PRIOS, p).astype(np.int64)
    nominated_node = np.full(p, -1, np.int64)
    self_id = np.full(p, -1, np.int64)
    for pos, (node, prio, rid) in zip(OWNER_POS, owner_rows):
        priority[pos], nominated_node[pos], self_id[pos] = prio, node, rid
    # the owner whose nominated node is full: nothing fits there
    full = int(nominated_node[FULL_OWNER])
    nodes.allowed_pods[full] = nodes.pod_count[full]
    # the owner its quota rejects
    w.pods.quota_req[synth.QDIM_CPU, QUOTA_OWNER] = 1 << 40
    return w, nom, priority, nominated_node, self_id


RESCAN_A, RESCAN_B, RESCAN_NOM = 3, 10, 20   # the two best open nodes of the chunk, the nominated node next to them


def rescan_workload(oracle_lib, n_pods: int = 12):
    """(w, nom, priority): one 64-node chunk of identical half-full nodes that pass LoadAware's Filter, two emptier
    ones (RESCAN_A, RESCAN_B) and the emptiest, RESCAN_NOM, whose room a row of priority 1000 holds; equal pods of
    priority 500, each 1/12 of a node.  The first two pods take A and B, so for every later pod the chunk's best and
    runner-up are both touched and their current keys lie below the runner-up's swept key: the commit re-scans the
    chunk's untouched nodes, among them the nominated node, which is closed to these pods."""
    w = synth.c2(n_nodes=64, n_pods=n_pods)
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ok = np.flatnonzero((orc.eval_pod(w.pods.rows([0]))[0] & ~np.uint32(FIT_BITS)) == 0)
    finally:
        orc.close()
    w.nodes = w.nodes.rows([int(ok[0])] * 64)
    nd = w.nodes
    nd.req_milli_cpu[:] = nd.nonzero_milli_cpu[:] = nd.alloc_milli_cpu // 2
    nd.req_memory[:] = nd.nonzero_memory[:] = nd.alloc_memory // 2
    nd.pod_count[:] = 10
    for i, div in ((RESCAN_A, 4), (RESCAN_B, 4), (RESCAN_NOM, 16)):
        nd.req_milli_cpu[i] = nd.nonzero_milli_cpu[i] = nd.alloc_milli_cpu[i] // div
        nd.req_memory[i] = nd.nonzero_memory[i] = nd.alloc_memory[i] // div
    cpu, mem = int(nd.alloc_milli_cpu[0]) // 12, int(nd.alloc_memory[0]) // 12
    w.pods.flags[:] = abi.KS_POD_PROD
    w.pods.req_milli_cpu[:] = w.pods.nonzero_milli_cpu[:] = w.pods.la_req_cpu[:] = cpu
    w.pods.req_memory[:] = w.pods.nonzero_memory[:] = w.pods.la_req_memory[:] = mem
    w.pods.quota_req[:] = 0
    nom = NominatedTable(1)
    nom.node[0], nom.priority[0], nom.id[0] = RESCAN_NOM, 1000, 5
    nom.req[0, 0] = room(nd, RESCAN_NOM) - cpu // 2   # half a pod's cpu is left
    return w, nom, np.full(n_pods, 500, np.int64)
