"""ks_eval_pod_summary (ks_summary.h: summary_block_kernel + summary_merge_kernel behind Evaluator.eval_pod_summary)
against numpy reductions of the CPU oracle's eval_pod, field by field and exactly: the feasible / unresolvable counts
and bitmasks, the per-reason-bit node counts, the winner and the top rows in (total descending, node ascending) order
with their score rows.  The expectation never comes from the device's own eval_pod.

Shapes sit where the kernels can go wrong: node counts around the 64-node bitmask word and the 256-node workgroup,
several workgroups with the winner in the last partial wave, all-equal totals, no feasible node, fewer feasible nodes
than rows asked for, reason words with bits 30 / 31 set (the topology branch), and the NUMA / DeviceShare profile."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_same_results
from koordinator_amd import abi, synth
from koordinator_amd.debug_scores import eval_debug_table, eval_debug_table_top

pytestmark = pytest.mark.gpu

TOPS = (0, 1, 5, 64)


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # the in-tree HIP library; no fallback
    return rt


def unpack(bits, n):
    """the bitmask words as bool [n]; the padding bits of the last word must be 0"""
    bits = np.asarray(bits, np.uint64)
    assert bits.shape == ((n + 63) // 64,)
    flat = np.unpackbits(bits.view(np.uint8), bitorder="little")
    assert not flat[n:].any(), "padding bits set"
    return flat[:n].astype(bool)


def want_summary(reasons, scores, total, top_n, mask):
    """the summary of one oracle evaluation (reasons [n], scores [n, plugins], total [n])"""
    reasons = np.asarray(reasons, np.uint32)
    n = len(reasons)
    feas = reasons == 0
    idx = np.flatnonzero(feas)
    order = idx[np.lexsort((idx, -np.asarray(total, np.int64)[idx]))]
    top = order[:top_n]
    return {
        "nodes": n, "feasible": int(feas.sum()), "unresolvable": int(((reasons & np.uint32(mask)) != 0).sum()),
        "reason_nodes": np.array([int(((reasons >> np.uint32(b)) & np.uint32(1)).sum()) for b in range(32)], np.int64),
        "best_node": int(order[0]) if len(order) else -1,
        "best_total": int(total[order[0]]) if len(order) else -1,
        "top_nodes": top.astype(np.int32), "top_totals": np.asarray(total, np.int64)[top],
        "top_scores": np.asarray(scores, np.int64)[top],
        "feasible_mask": feas, "unresolvable_mask": (reasons & np.uint32(mask)) != 0,
    }


def check(ev, orc, pod, top_n, mask=0, label=""):
    """eval_pod_summary on the device == the reduction of the oracle's eval_pod; returns (device dict, oracle reasons)"""
    r, s, t = orc.eval_pod(pod)
    want = want_summary(r, s, t, top_n, mask)
    got = ev.eval_pod_summary(pod, top_n=top_n, unresolvable_mask=mask, want_bits=True)
    n = len(r)
    for k in ("nodes", "feasible", "unresolvable", "best_node", "best_total"):
        assert got[k] == want[k], f"{label} top_n={top_n}: {k} {got[k]} != {want[k]}"
    assert got["reason_nodes"].dtype == np.int64 and got["reason_nodes"].shape == (32,)
    assert np.array_equal(got["reason_nodes"], want["reason_nodes"]), f"{label} top_n={top_n}: reason_nodes"
    assert len(got["top_nodes"]) == min(top_n, want["feasible"]), f"{label} top_n={top_n}: top_count"
    assert np.array_equal(got["top_nodes"], want["top_nodes"]), f"{label} top_n={top_n}: top_nodes"
    assert np.array_equal(got["top_totals"], want["top_totals"]), f"{label} top_n={top_n}: top_totals"
    assert got["top_scores"].shape == (len(want["top_nodes"]), abi.KS_NUM_SCORE_PLUGINS)
    assert np.array_equal(got["top_scores"], want["top_scores"]), f"{label} top_n={top_n}: top_scores"
    if top_n >= 1 and want["feasible"] >= 1:
        assert got["best_node"] == got["top_nodes"][0]
    assert np.array_equal(unpack(got["feasible_bits"], n), want["feasible_mask"]), f"{label}: feasible_bits"
    assert np.array_equal(unpack(got["unresolvable_bits"], n), want["unresolvable_mask"]), f"{label}: unresolvable_bits"
    return got, r


def pair(runtime, oracle_lib, w, nodes=None):
    nodes = w.nodes if nodes is None else nodes
    return (runtime.Evaluator(w.cfg, nodes.copy(), **w.tables()),
            oracle_lib.Oracle(w.cfg, nodes.copy(), **w.tables()))


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 257, 1000])
def test_tail_and_word_boundaries(runtime, oracle_lib, n_nodes):
    """node counts around the bitmask word and the workgroup, before anything is committed and after 20 commits"""
    w = synth.c2(n_nodes=n_nodes, n_pods=40)
    ev, orc = pair(runtime, oracle_lib, w)
    mask = abi.KS_R_FIT_CPU | abi.KS_R_LA_CPU
    try:
        for top_n in TOPS:
            check(ev, orc, w.pods.rows([0]), top_n, mask, f"n={n_nodes} fresh")
        head = w.pods.rows(list(range(20)))
        assert_same_results(ev.schedule(head), orc.schedule(head), f"n={n_nodes}")
        for top_n in TOPS:
            for i in (0, 20):
                check(ev, orc, w.pods.rows([i]), top_n, mask, f"n={n_nodes} after 20 commits, pod {i}")
    finally:
        ev.close()
        orc.close()


def test_multi_block_merge_winner_in_last_partial_wave(runtime, oracle_lib):
    """5000 nodes = 19 full workgroups + 136 nodes, whose last wave holds nodes 4992..4999: the last three nodes are
    emptied so that the winner and the runners-up come from that partial wave through the merge"""
    w = synth.c2(n_nodes=5000, n_pods=4)
    nd = w.nodes
    last = np.arange(4997, 5000)
    nd.alloc_milli_cpu[last] = 96_000
    nd.alloc_memory[last] = 512 << 30
    nd.la_alloc_milli_cpu[last] = nd.alloc_milli_cpu[last]
    nd.la_alloc_memory[last] = nd.alloc_memory[last]
    nd.la_total_milli_cpu[last] = nd.alloc_milli_cpu[last]
    nd.la_total_milli_memory[last] = nd.alloc_memory[last] * 1000
    for col in ("req_milli_cpu", "req_memory", "req_ephemeral", "nonzero_milli_cpu", "nonzero_memory", "pod_count",
                "la_term_milli_cpu", "la_term_memory", "la_prod_term_milli_cpu", "la_prod_term_memory",
                "la_usage_milli_cpu", "la_usage_milli_memory", "la_prod_usage_milli_cpu", "la_prod_usage_milli_memory"):
        getattr(nd, col)[last] = 0
    nd.req_scalar[:, last] = 0
    ev, orc = pair(runtime, oracle_lib, w)
    try:
        prod = int(np.flatnonzero((w.pods.flags & abi.KS_POD_PROD) != 0)[0])
        pod = w.pods.rows([prod])
        r, s, t = orc.eval_pod(pod)
        best = want_summary(r, s, t, 64, 0)
        assert best["best_node"] >= 4992, "the oracle's winner is not in the last partial wave"  # the case's premise
        assert len(best["top_nodes"]) == 64 and len(set(best["top_nodes"] // 256)) > 4  # rows of many workgroups
        check(ev, orc, pod, 64, abi.KS_R_LA_CPU | abi.KS_R_LA_MEMORY, "n=5000")
        check(ev, orc, pod, 0, 0, "n=5000")
    finally:
        ev.close()
        orc.close()


def test_all_ties(runtime, oracle_lib):
    """identical nodes: the order is the node order alone"""
    w = synth.c2(n_nodes=300, n_pods=4)
    nodes = w.nodes.rows([0] * 300)
    ev, orc = pair(runtime, oracle_lib, w, nodes)
    try:
        for i in range(4):
            got, r = check(ev, orc, w.pods.rows([i]), 64, 0, f"ties pod {i}")
            if (r == 0).all():
                assert got["best_node"] == 0
                assert np.array_equal(got["top_nodes"], np.arange(64))
                assert len(set(got["top_totals"].tolist())) == 1
                break
        else:
            pytest.fail("no pod of the four fits node 0")
    finally:
        ev.close()
        orc.close()


def big_pod(w):
    """pod 0 of a prod pod's row with CPU and memory requests above every node's allocatable"""
    prod = int(np.flatnonzero((w.pods.flags & abi.KS_POD_PROD) != 0)[0])
    pod = w.pods.rows([prod])
    pod.req_milli_cpu[:] = 10_000_000
    pod.req_memory[:] = 1 << 50
    pod.nonzero_milli_cpu[:] = pod.req_milli_cpu
    pod.nonzero_memory[:] = pod.req_memory
    return pod


def test_nothing_feasible(runtime, oracle_lib):
    n = 333
    w = synth.c2(n_nodes=n, n_pods=8)
    ev, orc = pair(runtime, oracle_lib, w)
    try:
        pod = big_pod(w)
        got, r = check(ev, orc, pod, 10, abi.KS_R_FIT_CPU, "nothing feasible")
        assert got["feasible"] == 0 and got["best_node"] == -1 and got["best_total"] == -1
        assert len(got["top_nodes"]) == 0 and got["top_scores"].shape == (0, abi.KS_NUM_SCORE_PLUGINS)
        # a node with two reasons counts under both
        assert got["reason_nodes"][abi.KS_R_FIT_CPU.bit_length() - 1] == n
        assert got["reason_nodes"][abi.KS_R_FIT_MEMORY.bit_length() - 1] == n
        assert got["unresolvable"] == n
        assert unpack(got["unresolvable_bits"], n).all()
        assert not unpack(got["feasible_bits"], n).any()
        # mask 0: no unresolvable node, all-zero words
        got0 = ev.eval_pod_summary(pod, top_n=0, unresolvable_mask=0, want_bits=True)
        assert got0["unresolvable"] == 0 and not got0["unresolvable_bits"].any()
    finally:
        ev.close()
        orc.close()


def test_top_n_larger_than_feasible(runtime, oracle_lib):
    """exactly 3 feasible nodes (a pod only three enlarged nodes hold), 10 rows asked for"""
    n = 400
    w = synth.c2(n_nodes=n, n_pods=8)
    keep = np.array([5, 260, 399])
    w.nodes.alloc_milli_cpu[keep] = 20_000_000
    w.nodes.alloc_memory[keep] = 1 << 52
    for col in ("la_term_milli_cpu", "la_term_memory", "la_prod_term_milli_cpu", "la_prod_term_memory",
                "la_usage_milli_cpu", "la_usage_milli_memory", "la_prod_usage_milli_cpu", "la_prod_usage_milli_memory"):
        getattr(w.nodes, col)[keep] = 0  # (no LoadAware threshold in the way)
    ev, orc = pair(runtime, oracle_lib, w)
    try:
        pod = big_pod(w)
        r, _, _ = orc.eval_pod(pod)
        assert np.array_equal(np.flatnonzero(r == 0), keep)  # the case's premise, on the oracle
        got, _ = check(ev, orc, pod, 10, abi.KS_R_FIT_MEMORY, "3 feasible")
        assert len(got["top_nodes"]) == 3 and got["feasible"] == 3
        assert sorted(got["top_nodes"].tolist()) == keep.tolist()
    finally:
        ev.close()
        orc.close()


def test_wide_reason_words_topology(runtime, oracle_lib):
    """the default profile with PodTopologySpread / InterPodAffinity (the shared topology branch): pods whose reason
    words carry bit 30 (pod anti-affinity) or bit 31 (existing pods' anti-affinity) on some node"""
    w = synth.with_topology(synth.c2_default(n_nodes=200, n_pods=60), seed=32)
    ev, orc = pair(runtime, oracle_lib, w)
    hi = abi.KS_R_POD_ANTI_AFFINITY | abi.KS_R_EXISTING_ANTI_AFFINITY
    seen = 0
    try:
        for i in range(w.pods.n):
            pod = w.pods.rows([i])
            r, _, _ = orc.eval_pod(pod)
            bits = int(np.bitwise_or.reduce(r)) & hi
            if not bits or (seen | bits) == seen:
                continue
            seen |= bits
            got, _ = check(ev, orc, pod, 5, hi, f"topology pod {i}")
            for b in (30, 31):
                assert got["reason_nodes"][b] == int(((r >> np.uint32(b)) & np.uint32(1)).sum())
            assert got["unresolvable"] == int(((r & np.uint32(hi)) != 0).sum()) > 0
            if seen == hi:
                break
    finally:
        ev.close()
        orc.close()
    assert seen & abi.KS_R_EXISTING_ANTI_AFFINITY, "no pod with bit 31 on any node: pick another seed"
    assert seen & abi.KS_R_POD_ANTI_AFFINITY, "no pod with bit 30 on any node: pick another seed"


def test_numa_deviceshare_profile(runtime, oracle_lib):
    """C3: the device and NUMA reason bits and the DeviceShare normalization"""
    w = synth.c3(n_nodes=120, n_pods=10)
    ev, orc = pair(runtime, oracle_lib, w)
    dev_numa = (abi.KS_R_DEV_INSUFFICIENT | abi.KS_R_DEV_NO_GPU | abi.KS_R_DEV_NO_RDMA | abi.KS_R_DEV_JOINT
                | abi.KS_R_NUMA_AMPLIFIED_CPU | abi.KS_R_NUMA_INVALID_TOPOLOGY | abi.KS_R_NUMA_AFFINITY
                | abi.KS_R_NUMA_INSUFFICIENT | abi.KS_R_NUMA_MISSING | abi.KS_R_NUMA_CPUSET)
    seen = 0
    try:
        for i in range(w.pods.n):
            _, r = check(ev, orc, w.pods.rows([i]), 16, dev_numa, f"c3 pod {i}")
            seen |= int(np.bitwise_or.reduce(r))
    finally:
        ev.close()
        orc.close()
    assert seen & dev_numa


def test_refusals_and_arguments(runtime):
    w = synth.c2(n_nodes=100, n_pods=4)
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    try:
        pod = w.pods.rows([0])
        for top_n in (-1, abi.KS_SUMMARY_MAX_TOP + 1):
            with pytest.raises(runtime.KsError) as e:
                ev.eval_pod_summary(pod, top_n=top_n)
            assert e.value.rc == abi.KS_EINVAL and "top_n" in str(e.value)
        cols = pod.ks()
        s = abi.KsPodSummary()
        rc = ev.L.ks_eval_pod_summary(ev.h, C.byref(cols), 0, 5, C.byref(s), None, None, None, None, None)
        assert rc == abi.KS_EINVAL and b"top_n" in ev.L.ks_last_error(ev.h)
        rc = ev.L.ks_eval_pod_summary(ev.h, C.byref(cols), 0, 0, None, None, None, None, None, None)
        assert rc == abi.KS_EINVAL and b"out" in ev.L.ks_last_error(ev.h)
        bad = w.pods.rows([0])
        bad.flags[:] |= abi.KS_POD_UNMODELLED
        with pytest.raises(runtime.KsError) as e:
            ev.eval_pod_summary(bad, top_n=1)
        assert e.value.rc == abi.KS_EUNSUPPORTED
        # the refused calls left the context usable
        assert ev.eval_pod_summary(pod, top_n=1)["nodes"] == 100
    finally:
        ev.close()
    empty = runtime.Evaluator(w.cfg)  # nothing loaded
    try:
        with pytest.raises(runtime.KsError) as e:
            empty.eval_pod_summary(w.pods.rows([0]), top_n=1)
        assert e.value.rc == abi.KS_ESTATE
    finally:
        empty.close()


def test_non_interference(runtime, oracle_lib):
    """eval_pod around a summary call returns the same arrays, and schedule after one still matches the oracle"""
    w = synth.c2(n_nodes=700, n_pods=60)
    ev, orc = pair(runtime, oracle_lib, w)
    try:
        pod = w.pods.rows([3])
        before = [a.copy() for a in ev.eval_pod(pod)]
        check(ev, orc, pod, 16, abi.KS_R_FIT_CPU, "non-interference")
        after = ev.eval_pod(pod)
        for a, b, o in zip(before, after, orc.eval_pod(pod)):
            assert np.array_equal(a, b) and np.array_equal(a, o)
        assert_same_results(ev.schedule(w.pods), orc.schedule(w.pods), "schedule after a summary")
        check(ev, orc, pod, 16, abi.KS_R_FIT_CPU, "after the schedule")
    finally:
        ev.close()
        orc.close()


def test_debug_table_from_the_summary(runtime, oracle_lib):
    """eval_debug_table_top (10 rows off the device) renders eval_debug_table's string, the oracle's too"""
    w = synth.with_static_plugins(synth.c1(n_nodes=300, n_pods=12), seed=31)
    cfg = w.cfg
    ev, orc = pair(runtime, oracle_lib, w)
    names = [f"node-{i}" for i in range(w.nodes.n)]
    shown = 0
    try:
        for i in range(w.pods.n):
            pod = w.pods.rows([i])
            got = eval_debug_table_top(ev, cfg, pod, names, 10, f"default/pod-{i}")
            assert got == eval_debug_table(ev, cfg, pod, names, 10, f"default/pod-{i}"), f"pod {i}"
            assert got == eval_debug_table(orc, cfg, pod, names, 10, f"default/pod-{i}"), f"pod {i} (oracle)"
            shown += got is not None
        assert eval_debug_table_top(ev, cfg, w.pods.rows([0]), names, 0, "default/pod-0") is None
    finally:
        ev.close()
        orc.close()
    assert shown > 0
