"""The staged prologue of the Fit + LoadAware + ElasticQuota commit kernel (ks_fq.h): the select kernel
writes one record per pod of the pass (the finished FqPod and the raw rows of the pod's top and second-best nodes; the
FqPod's quota words come from the per-call array prep_fq_words_kernel writes), and the commit loads the pass from that
record in one burst instead of gathering it.  KS_FQ_STAGED=0 (read when a context is created) keeps the gather
prologue.  ks_stats.diag[6] counts the passes the staged prologue loaded.

Every case schedules the same queues on the CPU oracle, on a default context and on a KS_FQ_STAGED=0 context, asserts
which prologue ran, and compares node, status and score of every pod, the node state, the quota `used` table and the
pass counters exactly.

Shapes: 130 nodes (three chunks, the last with 2 nodes) and 40 nodes (less than a chunk); 1, 63, 64, 65 and 130 pods
(a pass of one pod, a pass one short, a full pass, a second pass of one pod, a third pass of 2).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_same_results, assert_same_state, homogeneous_pods, profile
from koordinator_amd import abi, synth
from test_gpu_commit_fq import assert_edges, edge_workload, np_followup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("passes", "cut_passes", "rescans", "slot_misses", "bubble_passes")
Q_CPU, Q_MEM = synth.QDIM_CPU, synth.QDIM_MEMORY
STAGED = 6  # ks_stats.diag: passes the staged prologue loaded


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # must load the in-tree HIP library; no fallback
    return rt


def evaluator(runtime, cfg, nodes, quotas, vshards=1, pipeline=None, **env):
    """a context created with the given environment switches (read when a context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ev = runtime.Evaluator(cfg, nodes.copy(), quotas.copy())
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if pipeline is not None:
        ev.set_pipeline(pipeline)
    if vshards > 1:
        ev.shard(1, 0, None, vshards)
    return ev


def compare(tag, orc, dflt, gather, pods, staged):
    """one queue on the three; returns the oracle's results and the default context's stats"""
    want = orc.schedule(pods)
    got = dflt.schedule(pods)
    got_g = gather.schedule(pods)
    s_d, s_g = dflt.stats(), gather.stats()
    print(tag, {k: s_d[k] for k in COUNTERS}, "staged passes", s_d["diag"][STAGED], s_g["diag"][STAGED], "fast picks",
          s_d["diag"][7], "helpers", s_d["commit_helpers"], "LDS", s_d["commit_lds_bytes"])
    if staged:
        assert s_d["diag"][STAGED] == s_d["passes"] > 0, f"{tag}: the staged prologue did not load every pass"
    else:
        assert s_d["diag"][STAGED] == 0, f"{tag}: the staged prologue ran where the gather prologue was meant to"
    assert s_g["diag"][STAGED] == 0, f"{tag}: KS_FQ_STAGED=0 still ran the staged prologue"
    assert s_d["commit_helpers"] == s_g["commit_helpers"] and s_d["commit_lds_bytes"] == s_g["commit_lds_bytes"]
    assert_same_results(got, want, f"{tag} staged/oracle")
    assert_same_results(got, got_g, f"{tag} staged/gather")
    assert_same_state(dflt.read_nodes(), orc.read_nodes(), f"{tag} staged/oracle")
    assert_same_state(dflt.read_nodes(), gather.read_nodes(), f"{tag} staged/gather")
    assert np.array_equal(dflt.read_quota_used(), orc.read_quota_used()), f"{tag}: quota used differs from the oracle"
    assert np.array_equal(dflt.read_quota_used(), gather.read_quota_used()), f"{tag}: quota used differs between the two"
    for k in COUNTERS:
        assert s_d[k] == s_g[k], f"{tag}: counter {k} {s_d[k]} != {s_g[k]}"
    assert s_d["diag"][7] == s_g["diag"][7], f"{tag}: fast picks differ"
    return want, s_d


def both_ways(runtime, oracle_lib, prof, nodes, quotas, queues, label, staged=True, **ctx):
    """Schedules the queues one after the other on the oracle, the default path and the KS_FQ_STAGED=0 path; returns
    the oracle's results and the default path's stats per queue."""
    cfg = prof.to_ks_config()
    env = {k: ctx.pop(k) for k in list(ctx) if k.startswith("KS_")}
    orc = oracle_lib.Oracle(cfg, nodes.copy(), quotas.copy(), nthreads=4)
    dflt = evaluator(runtime, cfg, nodes, quotas, KS_FQ_STAGED="1", **env, **ctx)
    gather = evaluator(runtime, cfg, nodes, quotas, KS_FQ_STAGED="0", **env, **ctx)
    wants, stats = [], []
    try:
        for qi, pods in enumerate(queues):
            want, st = compare(f"{label} queue {qi}", orc, dflt, gather, pods, staged)
            wants.append(want)
            stats.append(st)
    finally:
        dflt.close()
        gather.close()
        orc.close()
    return wants, stats


def quota_pods(pods, rows):
    pods.quota[:] = np.arange(pods.n) % rows
    pods.quota_req[Q_CPU] = pods.req_milli_cpu
    pods.quota_req[Q_MEM] = pods.req_memory
    pods.quota_mask[:] = (1 << Q_CPU) | (1 << Q_MEM)
    return pods


@pytest.mark.parametrize("n_nodes", [130, 40])
@pytest.mark.parametrize("n_pods", [1, 63, 64, 65, 130])
def test_pass_lengths(runtime, oracle_lib, n_nodes, n_pods):
    """the last pass short, and the record's pod index across passes"""
    rng = np.random.Generator(np.random.PCG64(1000 + n_nodes + n_pods))
    nodes = synth.make_nodes(n_nodes, rng)
    pods = synth.make_pods(n_pods, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = synth.make_quotas(pods, 4, rng, admit_frac=0.8)
    _, stats = both_ways(runtime, oracle_lib, profile(quota=True, check_parent=True), nodes, q, [pods],
                         f"n{n_nodes}-p{n_pods}")
    assert stats[0]["passes"] >= (n_pods + 63) // 64


def test_cut_passes_restart_at_the_cut(runtime, oracle_lib):
    """2 candidates and identical pods on 192 nodes: passes are cut, and the pass after a cut starts at a cursor the
    cut pass's select did not assume, so its records must be those of the re-swept pods"""
    rng = np.random.Generator(np.random.PCG64(4))
    nodes = synth.make_nodes(192, rng)
    pods = quota_pods(homogeneous_pods(130), 3)
    q = synth.make_quotas(pods, 3, rng, admit_frac=0.95)
    _, stats = both_ways(runtime, oracle_lib, profile(quota=True, candidates=2), nodes, q, [pods], "cut")
    assert stats[0]["cut_passes"] > 0
    assert stats[0]["passes"] > 3


def test_quota_tree_rejections_and_pods_without_quota(runtime, oracle_lib):
    """a three-level quota chain with the ancestor check on (qmeta's parent and masks come from the per-call words),
    leaves that fill up inside a pass, non-preemptible pods against `min`, pods without a quota; then a queue that
    depends on the usage the first one left"""
    nodes, pods, q = edge_workload()
    wants, _ = both_ways(runtime, oracle_lib, profile(quota=True, check_parent=True), nodes, q,
                         [pods, np_followup(pods)], "tree")
    assert_edges(wants[0], pods)
    s1 = np.asarray(wants[1]["status"])
    assert (s1 == abi.KS_S_QUOTA_NONPREEMPTIBLE).any() and (s1 == abi.KS_S_SCHEDULED).any()


def test_one_feasible_node_and_none(runtime, oracle_lib):
    """40 nodes, 64 pods: three pods fit one node only (no second-best node: a zero second row), and once the first
    of them is on it the others find their only node touched and no other; one pod fits no node (no top: a zero top
    row)"""
    rng = np.random.Generator(np.random.PCG64(1234))
    nodes = synth.make_nodes(40, rng)
    pods = synth.make_pods(64, rng, 3)
    nodes.alloc_memory[3] = 1 << 47
    nodes.la_alloc_memory[3] = 1 << 47
    big = [10, 20, 30]
    pods.req_memory[big] = pods.nonzero_memory[big] = 3 << 45
    pods.req_milli_cpu[29] = pods.nonzero_milli_cpu[29] = 10 ** 9
    pods.quota[big + [29]] = -1
    q = synth.make_quotas(pods, 3, rng, admit_frac=2.0)
    prof = profile(quota=True)
    orc = oracle_lib.Oracle(prof.to_ks_config(), nodes.copy(), q.copy(), nthreads=1)
    feasible = [int((orc.eval_pod(pods.rows(np.array([j])))[0] == 0).sum()) for j in big + [29]]
    orc.close()
    assert feasible == [1, 1, 1, 0], "the snapshot was meant to give three pods one feasible node and one pod none"
    wants, _ = both_ways(runtime, oracle_lib, prof, nodes, q, [pods], "one-or-none")
    stt, node = np.asarray(wants[0]["status"]), np.asarray(wants[0]["node"])
    assert stt[10] == abi.KS_S_SCHEDULED and node[10] == 3
    assert stt[20] == stt[30] == stt[29] == abi.KS_S_UNSCHEDULABLE


def test_quota_table_reloaded_between_calls(runtime, oracle_lib):
    """one context: a queue under table A, then the nodes and table B loaded (other parents, other masks), the same
    queue again -- against a fresh oracle on B, so the per-call words cannot be table A's"""
    nodes, pods, qa = edge_workload()
    qb = qa.copy()
    qb.parent[0] = -1      # leaf 0 leaves the chain
    qb.parent[1] = 5       # leaf 1 hangs under the top directly
    qb.parent[3] = 4       # leaf 3 joins it
    qb.limit_mask[2] = 0   # leaf 2 limits nothing any more
    qb.min_mask[3] = 0
    prof = profile(quota=True, check_parent=True)
    cfg = prof.to_ks_config()
    orc_a = oracle_lib.Oracle(cfg, nodes.copy(), qa.copy(), nthreads=4)
    orc_b = oracle_lib.Oracle(cfg, nodes.copy(), qb.copy(), nthreads=4)
    dflt = evaluator(runtime, cfg, nodes, qa, KS_FQ_STAGED="1")
    gather = evaluator(runtime, cfg, nodes, qa, KS_FQ_STAGED="0")
    try:
        want_a, _ = compare("reload A", orc_a, dflt, gather, pods, True)
        for ev in (dflt, gather):
            ev.load_nodes(nodes.copy())
            ev.load_quotas(qb.copy())
        want_b, _ = compare("reload B", orc_b, dflt, gather, pods, True)
    finally:
        dflt.close()
        gather.close()
        orc_a.close()
        orc_b.close()
    sa, sb = np.asarray(want_a["status"]), np.asarray(want_b["status"])
    assert (sa != sb).any(), "the two tables were meant to admit different pods"
    assert ((sa == abi.KS_S_QUOTA) & (sb == abi.KS_S_SCHEDULED) & (pods.quota == 2)).any(), "leaf 2's dropped limit mask"
    assert ((sa & abi.KS_S_QUOTA_PARENT) != (sb & abi.KS_S_QUOTA_PARENT)).any(), "the changed parents"


def test_builder_only_variant_reads_the_same_record(runtime, oracle_lib):
    """KS_FQ_KEYS=0: commit_fq_kernel<NSC, false> (wave 0 evaluates the touched slots) with the staged prologue"""
    rng = np.random.Generator(np.random.PCG64(9))
    nodes = synth.make_nodes(40, rng)
    pods = synth.make_pods(130, rng, 2)
    q = synth.make_quotas(pods, 2, rng, admit_frac=2.0)
    _, stats = both_ways(runtime, oracle_lib, profile(quota=True), nodes, q, [pods], "keys0", KS_FQ_KEYS="0")
    assert stats[0]["commit_helpers"] == 0, "KS_FQ_KEYS=0 still ran the evaluating helper waves"


def test_two_virtual_shards_keep_the_gather_prologue(runtime, oracle_lib):
    """vshards = 2: the merge kernel finalises the lists and writes no record, so the commit gathers"""
    rng = np.random.Generator(np.random.PCG64(41))
    nodes = synth.make_nodes(130, rng)
    pods = synth.make_pods(130, rng, 4)
    pods.flags[::9] |= abi.KS_POD_NONPREEMPTIBLE
    q = synth.make_quotas(pods, 4, rng, admit_frac=0.7)
    wants, _ = both_ways(runtime, oracle_lib, profile(quota=True, check_parent=True), nodes, q, [pods], "vshards",
                         staged=False, vshards=2)
    assert (np.asarray(wants[0]["status"]) & abi.KS_S_QUOTA).any()


# The re-swept pipeline runs the dedicated kernel only with KS_PIPE_PATCH=0 (a monotone profile is patched
# otherwise, and patched passes run the general commit), and that switch is read once per process: a child process.
RESWEPT_CHILD = r"""
import numpy as np
from helpers import homogeneous_pods, profile
from koordinator_amd import synth
from oracle import oracle
import test_gpu_commit_fq_staged as t
from koordinator_amd import runtime

oracle.build()
rng = np.random.Generator(np.random.PCG64(11))
nodes = synth.make_nodes(192, rng)
pods = t.quota_pods(homogeneous_pods(200), 3)
q = synth.make_quotas(pods, 3, rng, admit_frac=0.95)
_, stats = t.both_ways(runtime, oracle, profile(quota=True, candidates=2), nodes, q, [pods], "re-swept", pipeline=2)
st = stats[0]
assert st["pipelined"] == 1, st
assert st["cut_passes"] > 0 and st["bubble_passes"] > 0, st
print("RESWEPT OK")
"""


def test_reswept_pipeline_on_a_small_cluster():
    """the select runs behind the fix sweep, for the pods of the pass's own start word; a pass after a cut is a bubble
    and its record is not applied"""
    env = dict(os.environ, KS_PIPE_PATCH="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + env.get("PYTHONPATH", "").split(os.pathsep))
    r = subprocess.run([sys.executable, "-c", RESWEPT_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "RESWEPT OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
