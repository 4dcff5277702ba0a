"""The helper waves' hand-offs of the Fit + LoadAware + ElasticQuota commit kernel (ks_fq.h, variant with the slot-key
table).  Wave 0 issues one descriptor per row change: a `build` descriptor for a new slot whose row was prefetched (a
helper wave builds the row and evaluates it at once), a `built` descriptor for a row it finished itself.  Waves 1 and 2
take alternate descriptors, each with its own counter, and wave 0 waits for both.  Every case compares node, status
and score of every pod (and the node state and the quota `used` table) exactly against the CPU oracle on the same
inputs, and against contexts of the same library with KS_FQ_KEYS=0 (wave 0 evaluates the touched slots) and with
KS_COMMIT_FQ=0 (the general commit kernel); the pass counters must agree between the three device paths.

Each case names the hand-off it is there for, and asserts with the oracle alone that its inputs produce it
(`first_pass`): the first pass's sweep sees the initial state, so `Oracle.eval_pod` before anything is scheduled gives
every pod's snapshot scores, and the oracle's placements say which nodes the pods before it touched.  From those:
  fast     the pod's snapshot-best node is untouched: a build descriptor (a helper builds and evaluates the row)
  second   slow pod onto its untouched snapshot second-best node: a build descriptor
  touched  slow pod onto a node an earlier pod of the pass took: a Reserve onto a slot, a built descriptor
  miss     slow pod onto another untouched node: wave 0 builds the row, a built descriptor
  chained  slow pod right behind a pod that issued a build descriptor (the creation followed at once by a read)
A pass is cut at a slow pod whose winner's key is below the bound of its candidate list.  The list holds
K chunks of the pod's snapshot: those whose best score is above the K-th best chunk score, then chunks at that score
in chunk order; the bound is the best key of the last chunk taken.  The walk stops at the first such pod.

Shapes: 64-pod passes, 2 or 3 node chunks (128 / 192 nodes), 40 nodes where slots must be reused.
"""
import os

import numpy as np
import pytest

from helpers import assert_same_results, assert_same_state, homogeneous_pods, profile
from koordinator_amd import abi, synth
from koordinator_amd.config import (BATCH_CPU, BATCH_MEMORY, CPU, MEMORY, ElasticQuotaArgs, LoadAwareSchedulingArgs,
                                    NodeResourcesFitArgs, SchedulerProfile)
from test_gpu_commit_fq import assert_edges, edge_workload, np_followup
from test_gpu_commit_fq_keys import divergent_workload

pytestmark = pytest.mark.gpu

COLS = ("node", "status", "score", "reservation", "gpu_minors", "rdma_minors")
COUNTERS = ("passes", "cut_passes", "rescans", "slot_misses", "bubble_passes")
Q_CPU, Q_MEM = synth.QDIM_CPU, synth.QDIM_MEMORY
KEYS_RAN = 2  # ks_stats.commit_helpers: the helper waves evaluated the slot keys
BATCH = 64


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # must load the in-tree HIP library; no fallback
    return rt


def evaluator(runtime, cfg, nodes, quotas, **env):
    """a context created with the given environment switches (both are read when a context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return runtime.Evaluator(cfg, nodes.copy(), quotas.copy())
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def four_way(runtime, oracle_lib, prof, nodes, quotas, queues, label, table_fits=True):
    """Schedules the queues one after the other on the oracle, the default path, the KS_FQ_KEYS=0 path and the
    KS_COMMIT_FQ=0 path; returns the oracle's results per queue and the default path's stats per queue."""
    cfg = prof.to_ks_config()
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas.copy(), nthreads=4)
    dflt = evaluator(runtime, cfg, nodes, quotas, KS_FQ_KEYS="1", KS_COMMIT_FQ="1")
    others = {"KS_FQ_KEYS=0": evaluator(runtime, cfg, nodes, quotas, KS_FQ_KEYS="0", KS_COMMIT_FQ="1"),
              "KS_COMMIT_FQ=0": evaluator(runtime, cfg, nodes, quotas, KS_COMMIT_FQ="0")}
    wants, stats = [], []
    try:
        for qi, pods in enumerate(queues):
            tag = f"{label} queue {qi}"
            want = orc.schedule(pods)
            got = dflt.schedule(pods)
            s_d = dflt.stats()
            print(tag, {k: s_d[k] for k in COUNTERS}, "fast picks", s_d["diag"][7], "helpers", s_d["commit_helpers"],
                  "LDS", s_d["commit_lds_bytes"])
            if table_fits:
                assert s_d["commit_helpers"] == KEYS_RAN, f"{tag}: the default path did not run the slot-key variant"
            else:
                assert s_d["commit_helpers"] != KEYS_RAN, f"{tag}: the slot-key variant ran without room for its table"
            assert s_d["commit_lds_bytes"] <= 160 * 1024
            assert_same_results(got, want, f"{tag} default/oracle")
            for k in COLS:
                assert np.array_equal(got[k], want[k]), f"{tag}: {k} differs from the oracle"
            assert_same_state(dflt.read_nodes(), orc.read_nodes(), f"{tag} default/oracle")
            assert np.array_equal(dflt.read_quota_used(), orc.read_quota_used()), f"{tag}: quota used differs from the oracle"
            for name, ev in others.items():
                got_o = ev.schedule(pods)
                s_o = ev.stats()
                assert s_o["commit_helpers"] != KEYS_RAN, f"{tag}: {name} still ran the slot-key variant"
                for k in COLS:
                    assert np.array_equal(got[k], got_o[k]), f"{tag}: {k} differs from the {name} path"
                assert_same_state(dflt.read_nodes(), ev.read_nodes(), f"{tag} default/{name}")
                assert np.array_equal(dflt.read_quota_used(), ev.read_quota_used()), f"{tag}: quota used differs from {name}"
                for k in COUNTERS:
                    assert s_d[k] == s_o[k], f"{tag}: counter {k} {s_d[k]} != {s_o[k]} ({name})"
                assert s_d["diag"][7] == s_o["diag"][7], f"{tag}: fast picks differ from {name}"
            wants.append(want)
            stats.append(s_d)
    finally:
        dflt.close()
        for ev in others.values():
            ev.close()
        orc.close()
    return wants, stats


def first_pass(oracle_lib, prof, nodes, quotas, pods):
    """The first pass's hand-offs by the oracle alone (module docstring): counts per class of the pods walked, the
    walked pods' classes in order, and `cut` = the pass position of a certain cut (None: the walk ended otherwise)."""
    cfg = prof.to_ks_config()
    k = prof.candidates if prof.candidates > 0 else 32
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas.copy(), nthreads=1)
    npass = min(BATCH, pods.n)
    snap = []
    for j in range(npass):
        reasons, _, total = orc.eval_pod(pods.rows(np.array([j])))
        snap.append(np.where(reasons == 0, total, -1))
    want = orc.schedule(pods)
    orc.close()
    nchunks = (nodes.n + 63) // 64
    classes, touched, cut = [], set(), None
    for j in range(npass):
        st, node, score = int(want["status"][j]), int(want["node"][j]), int(want["score"][j])
        if st != abi.KS_S_SCHEDULED:
            classes.append("rejected")
            continue
        tot = snap[j]
        order = np.lexsort((np.arange(nodes.n), -tot))  # best key first: score, then the lower node
        top, second = int(order[0]), int(order[1])
        if top not in touched:
            assert node == top and score == tot[top], "a monotone profile's untouched snapshot-best node wins"
            classes.append("fast")
            touched.add(node)
            continue
        cbest = np.array([tot[c * 64:(c + 1) * 64].max() for c in range(nchunks)])
        if (cbest >= 0).sum() > k:
            # the list: every chunk whose best score is above the K-th best one, then chunks at it in chunk order;
            # the bound is the best key of the last chunk taken
            t = np.sort(cbest)[::-1][k - 1]
            last = np.nonzero(cbest == t)[0][k - int((cbest > t).sum()) - 1]
            bound_node = last * 64 + int(np.argmax(tot[last * 64:(last + 1) * 64]))
            if (score, -node) < (int(t), -bound_node):
                cut = j
                break
        if node in touched:
            classes.append("touched")
        elif node == second:
            classes.append("second")
        else:
            classes.append("miss")
        touched.add(node)
    counts = {c: classes.count(c) for c in ("fast", "second", "touched", "miss", "rejected")}
    counts["chained"] = sum(1 for a, b in zip(classes, classes[1:])
                            if a in ("fast", "second") and b in ("second", "touched", "miss"))
    return counts, classes, cut


def quota_pods(pods, rows):
    pods.quota[:] = np.arange(pods.n) % rows
    pods.quota_req[Q_CPU] = pods.req_milli_cpu
    pods.quota_req[Q_MEM] = pods.req_memory
    pods.quota_mask[:] = (1 << Q_CPU) | (1 << Q_MEM)
    return pods


def test_slow_pods_on_prefetched_second_best(runtime, oracle_lib):
    """A helper's creation followed at once by a slow pod's read.  128 nodes (2 chunks), 130 identical pods with
    quotas: every pod has the same snapshot order of the nodes, so every pod after a pass's first is slow, and it lands
    on its second-best node (a helper builds and evaluates the row) or on a touched slot (a helper evaluates it)."""
    rng = np.random.Generator(np.random.PCG64(11))
    nodes = synth.make_nodes(128, rng)
    pods = quota_pods(homogeneous_pods(130), 3)
    q = synth.make_quotas(pods, 3, rng, admit_frac=2.0)
    prof = profile(quota=True)
    counts, classes, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    print("first pass", counts)
    assert cut is None and len(classes) == BATCH
    assert counts["fast"] == 1 and counts["rejected"] == 0, "identical pods: only the pass's first pod is fast"
    assert counts["second"] >= 1 and counts["touched"] >= 1
    assert counts["second"] + counts["touched"] > BATCH // 2, "the slow pods were meant for second-best nodes and slots"
    assert counts["chained"] >= 2, "no slow pod right behind each kind of creation by a helper (top and second-best row)"
    _, stats = four_way(runtime, oracle_lib, prof, nodes, q, [pods], "second-best")
    assert stats[0]["cut_passes"] == 0 and stats[0]["passes"] == 3


def test_misses_and_a_cut_with_descriptors_pending(runtime, oracle_lib):
    """Rows wave 0 builds itself, and `hdone` while descriptors are pending.  2 candidates per pod on 192 nodes (3 chunks) with
    identical pods: the third chunk is outside every list, slow pods land on touched slots and on untouched nodes that
    are not their second-best (rows wave 0 builds itself), and the first pass is cut inside it."""
    rng = np.random.Generator(np.random.PCG64(4))
    nodes = synth.make_nodes(192, rng)
    pods = quota_pods(homogeneous_pods(130), 3)
    q = synth.make_quotas(pods, 3, rng, admit_frac=0.95)
    prof = profile(quota=True, candidates=2)
    counts, classes, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    print("first pass", counts, "cut at", cut)
    assert cut is not None and 0 < cut < BATCH, "the first pass was meant to be cut inside"
    assert counts["touched"] + counts["miss"] >= 1, "no built descriptor before the cut"
    assert classes[cut - 1] in ("fast", "second", "touched", "miss"), "no descriptor issued right before the cut"
    _, stats = four_way(runtime, oracle_lib, prof, nodes, q, [pods], "misses-cut")
    assert stats[0]["cut_passes"] > 0
    assert stats[0]["slot_misses"] > 0, "no row built by wave 0"


def test_partial_last_pass_and_one_pod_queue(runtime, oracle_lib):
    """70 pods: the last pass has 6, so the helpers' lanes past the pass's pods must not store; then a queue of one
    pod on the same contexts (a pass whose only descriptor is its last, so wave 2 takes none)."""
    rng = np.random.Generator(np.random.PCG64(5))
    nodes = synth.make_nodes(128, rng)
    pods = synth.make_pods(70, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = synth.make_quotas(pods, 4, rng, admit_frac=1.5)
    one = quota_pods(homogeneous_pods(1), 1)
    prof = profile(quota=True, check_parent=True)
    counts, classes, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    print("first pass", counts)
    assert cut is None and len(classes) == BATCH
    assert counts["fast"] >= 1 and counts["second"] + counts["touched"] + counts["miss"] >= 1
    wants, stats = four_way(runtime, oracle_lib, prof, nodes, q, [pods, one], "tail")
    assert stats[0]["passes"] == 2, "64 + 6 pods, no cut with both chunks listed"
    assert stats[1]["passes"] == 1  # (the counters are per queue)
    assert (np.asarray(wants[0]["status"])[BATCH:] == abi.KS_S_SCHEDULED).any()
    assert int(wants[1]["status"][0]) == abi.KS_S_SCHEDULED


@pytest.mark.parametrize("nsc", [0, 2, 4])
def test_scalar_slot_variants(runtime, oracle_lib, nsc):
    """commit_fq_kernel<0|2|4, true>: 40 nodes, 64 pods whose evaluation takes a different path per lane (PROD and
    non-PROD, DaemonSet, zero requests, int64-path capacities), new slots and reused ones"""
    nodes, pods = divergent_workload(nsc)
    res = {CPU: 1, MEMORY: 1, BATCH_CPU: 1, BATCH_MEMORY: 1} if nsc else {CPU: 1, MEMORY: 1}
    prof = SchedulerProfile(fit=NodeResourcesFitArgs(strategy="LeastAllocated", resources=res), fit_weight=1,
                            loadaware=LoadAwareSchedulingArgs(score_according_prod_usage=True), loadaware_weight=1,
                            quota=ElasticQuotaArgs(enable_check_parent_quota=False))
    q = synth.make_quotas(pods, 3, np.random.Generator(np.random.PCG64(8)), admit_frac=2.0)
    counts, classes, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    print("first pass", counts)
    assert cut is None and len(classes) == BATCH
    assert counts["fast"] + counts["second"] >= 1, "no row for a helper to build"
    assert counts["touched"] >= 1, "no Reserve onto a touched slot"
    assert counts["chained"] >= 1
    four_way(runtime, oracle_lib, prof, nodes, q, [pods], f"nsc{nsc}")


def test_quota_rejections_mid_pass(runtime, oracle_lib):
    """A leaf that fills up inside the first pass (rejected pods issue nothing, smaller ones behind them still do), an
    ancestor's limit, and non-preemptible pods against `min`, here and in a follow-up queue that depends on the
    `npused` the first one left"""
    nodes, pods, q = edge_workload()
    prof = profile(quota=True, check_parent=True)
    cfg = prof.to_ks_config()
    orc = oracle_lib.Oracle(cfg, nodes.copy(), q.copy(), nthreads=1)
    want = orc.schedule(pods)
    s1 = np.asarray(orc.schedule(np_followup(pods))["status"])
    orc.close()
    assert_edges(want, pods)
    assert (s1 == abi.KS_S_QUOTA_NONPREEMPTIBLE).any() and (s1 == abi.KS_S_SCHEDULED).any()
    counts, classes, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    print("first pass", counts)
    assert cut is None and len(classes) == BATCH
    rej = [i for i, c in enumerate(classes) if c == "rejected"]
    assert rej and any(c != "rejected" for c in classes[rej[0]:]), "no rejection with placements behind it in the pass"
    assert counts["second"] + counts["touched"] + counts["miss"] >= 1
    four_way(runtime, oracle_lib, prof, nodes, q, [pods, np_followup(pods)], "quota")


def test_table_does_not_fit(runtime, oracle_lib):
    """64 candidates: the commit image has no room for the slot-key table, so the context keeps the in-wave
    evaluation (wave 1 builds only), and the results are still exact"""
    rng = np.random.Generator(np.random.PCG64(21))
    nodes = synth.make_nodes(128, rng)
    pods = quota_pods(homogeneous_pods(70), 3)
    q = synth.make_quotas(pods, 3, rng, admit_frac=2.0)
    prof = profile(quota=True, candidates=64)
    counts, _, cut = first_pass(oracle_lib, prof, nodes, q, pods)
    assert cut is None and counts["second"] + counts["touched"] >= 1
    four_way(runtime, oracle_lib, prof, nodes, q, [pods], "cand64", table_fits=False)
