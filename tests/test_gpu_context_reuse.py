"""A ks_ctx kept across table reloads (include/koordgpu.h, "Reusing a context"): a context built on workload A,
with commits, is moved to workload B by ks_load_nodes and the loads after it, single tables are replaced on a live
context, and the dependent tables are loaded in every order.  After each sequence the context must be what a fresh
context would be: the expectation is always a *fresh* CPU oracle built from the final tables (never the device's own
output), compared exactly -- placements, statuses, scores, nominated reservations, minors, node state and every
table's read-back, ks_eval_pod on five pods and ks_eval_pod_summary on one.

The scenarios' workloads come from reuse_util.py; test_context_reuse_premises.py shows on the oracle alone that
each reaches the cache or buffer it is about (DESIGN.md §7b lists them per table struct of ks_ctx)."""
import numpy as np
import pytest

import reuse_util as ru
from helpers import assert_same_results, assert_same_state
from koordinator_amd import abi
from test_gpu_eval_summary import check as check_summary

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # the in-tree HIP library; no fallback
    return rt


def tables_of(w, **over):
    t = w.tables()
    t.update(over)
    return {k: v for k, v in t.items() if v is not None}


def fresh(oracle_lib, cfg, w, **over):
    return oracle_lib.Oracle(cfg, w.nodes.copy(), nthreads=8, **tables_of(w, **over))


LOADERS = {"quotas": "load_quotas", "reservations": "load_reservations", "devices": "load_devices",
           "cpu_state": "load_cpu_state", "numa_nodes": "load_numa_nodes"}


def load_tables(ev, w, order=("quotas",) + ru.DEPENDENT, **over):
    t = tables_of(w, **over)
    for k in order:
        if k in t:
            getattr(ev, LOADERS[k])(t[k].copy())


def same_tables(ev, orc, t, label, npods=None):
    assert_same_state(ev.read_nodes(), orc.read_nodes(), label)
    if "quotas" in t:
        assert np.array_equal(ev.read_quota_used(), orc.read_quota_used()), f"{label}: quota used"
    if "devices" in t:
        for a, b in zip(ev.read_devices(), orc.read_devices()):
            assert np.array_equal(a, b), f"{label}: device usage"
    if "reservations" in t:
        for a, b in zip(ev.read_reservations(), orc.read_reservations()):
            assert np.array_equal(a, b), f"{label}: reservation allocated / assigned"
        assert np.array_equal(ev.read_reservation_devices(), orc.read_reservation_devices()), f"{label}: reservation devices"
    if "cpu_state" in t:
        for a, b in zip(ev.read_cpu_state(), orc.read_cpu_state()):
            assert np.array_equal(a, b), f"{label}: CPU state"
    if "numa_nodes" in t:
        for a, b in zip(ev.read_numa_nodes(), orc.read_numa_nodes()):
            assert np.array_equal(a, b), f"{label}: NUMA used"
    if npods is not None and "cpu_state" in t:
        assert np.array_equal(ev.fetch_cpusets(npods), orc.fetch_cpusets(npods)), f"{label}: cpusets"
    if npods is not None and "numa_nodes" in t:
        assert np.array_equal(ev.fetch_numa_alloc(npods), orc.fetch_numa_alloc(npods)), f"{label}: NUMA allocations"


def same_as_fresh(ev, orc, pods, t, label, schedule=None):
    """the context against the fresh oracle: the loaded state, single-pod evaluation, then the queue and what it left"""
    same_tables(ev, orc, t, label + " (loaded)")
    for i in np.linspace(0, pods.n - 1, 5).astype(int):
        pod = pods.rows([int(i)])
        for a, b, what in zip(ev.eval_pod(pod), orc.eval_pod(pod), ("reasons", "scores", "total")):
            assert np.array_equal(a, b), f"{label}: eval_pod {what} of pod {i}"
    check_summary(ev, orc, pods.rows([pods.n // 3]), 5, label=label)
    got = ev.schedule(pods) if schedule is None else schedule(pods)
    want = orc.schedule(pods)
    assert_same_results(got, want, label)
    for k in ("reservation", "gpu_minors", "rdma_minors"):
        assert np.array_equal(got[k], want[k]), f"{label}: {k}"
    same_tables(ev, orc, t, label, pods.n)
    return got


def start_on(runtime, oracle_lib, a, setup=None):
    """a context on A with the first half of A's queue committed and ks_read_nodes called once; the oracle that made
    the same commits"""
    ev = runtime.Evaluator(a.cfg)
    if setup:
        setup(ev)
    ev.load_nodes(a.nodes.copy())
    load_tables(ev, a)
    orc = fresh(oracle_lib, a.cfg, a)
    half = ru.first_half(a)
    assert_same_results(ev.schedule(half), orc.schedule(half), "A")
    assert_same_state(ev.read_nodes(), orc.read_nodes(), "A")
    return ev, orc


def move_to(ev, oracle_lib, cfg, b, label, order=ru.DEPENDENT, **over):
    """ks_load_nodes(B) and B's other tables on the live context, then everything against a fresh oracle"""
    ev.load_nodes(b.nodes.copy())
    load_tables(ev, b, order=order, **over)
    orc = fresh(oracle_lib, cfg, b, **over)
    try:
        return same_as_fresh(ev, orc, b.pods, tables_of(b, **over), label)
    finally:
        orc.close()


def test_r1_held_nodes_become_policy_nodes_without_a_reservation_reload(runtime, oracle_lib):
    """h_dev_held / dev_held_any / the FEAT 23 and 31 kernels: A's reservations hold devices; B puts a NUMA policy on
    those nodes and loads devices and NUMA nodes but no reservations, so no node may count as held any more"""
    a, b, _ = ru.r1()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        move_to(ev, oracle_lib, a.cfg, b, "R1")
        assert ev.read_reservations()[0].shape[0] == 0
    finally:
        ev.close()
        orc.close()


def test_r2_reservations_on_a_grown_cluster(runtime, oracle_lib):
    """rdscratch (ks_read_nodes' copy of the restored columns, sized by the padded node count), h_rsv_node, rsv_perm:
    150 -> 600 nodes, ks_read_nodes on both"""
    a, b = ru.r2()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        move_to(ev, oracle_lib, a.cfg, b, "R2")
    finally:
        ev.close()
        orc.close()


def test_r3_numa_counts_of_the_old_cluster(runtime, oracle_lib):
    """h_numa_k / check_dev_numa: A has 4-NUMA and 2-NUMA policy rows; B is larger, has no policy node and its
    devices sit on NUMA nodes 2 and 3 -- the old rows would refuse them (and rows past the old count do not exist)"""
    a, b, _ = ru.r3()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        move_to(ev, oracle_lib, a.cfg, b, "R3")
    finally:
        ev.close()
        orc.close()


def test_r4_wide_numa_then_device_holding_reservations(runtime, oracle_lib):
    """numa_w: after an 8-NUMA cluster (wide kernels) a cluster without any policy node must take reservations that
    hold devices (the FEAT 31 kernels exist at width 4 only) and run the narrow kernels"""
    a, b, _ = ru.r4()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        move_to(ev, oracle_lib, a.cfg, b, "R4")
    finally:
        ev.close()
        orc.close()


def test_r5_shrinking_cluster_keeps_quotas(runtime, oracle_lib):
    """1000 -> 65 -> 1 nodes (evbuf, sumbuf, the bitmask padding bits, sweep_out, the select kernel's LDS size);
    ks_load_nodes keeps the quota table with the usage of the commits so far"""
    a, b, c = ru.r5()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        ev.eval_pod_summary(a.pods.rows([0]), top_n=5, want_bits=True)  # sumbuf at 1000 nodes
        kept = ru.keep_quotas(a.quotas, orc)
        ev.load_nodes(b.nodes.copy())
        ob = fresh(oracle_lib, a.cfg, b, quotas=kept)
        same_as_fresh(ev, ob, b.pods, {"quotas": kept}, "R5 65 nodes")
        kept = ru.keep_quotas(kept, ob)
        ob.close()
        ev.load_nodes(c.nodes.copy())
        oc = fresh(oracle_lib, a.cfg, c, quotas=kept)
        same_as_fresh(ev, oc, c.pods, {"quotas": kept}, "R5 1 node")
        oc.close()
    finally:
        ev.close()
        orc.close()


def test_r6_cpu_state_not_reloaded(runtime, oracle_lib):
    """cpu_loaded / h_cpu_nn / the cpu_free = -1 column: the same nodes again, devices and NUMA nodes loaded, the CPU
    state not: no node has a CPU topology, so no cpu-bind pod fits and nothing of A's cpusets shows"""
    a, b = ru.r6()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        got = move_to(ev, oracle_lib, a.cfg, b, "R6")
        bind = (b.pods.flags & abi.KS_POD_CPU_BIND) != 0
        assert not (got["status"][bind] == abi.KS_S_SCHEDULED).any()
        assert not ev.fetch_cpusets(b.pods.n).any()
        assert not any(x.any() for x in ev.read_cpu_state())
    finally:
        ev.close()
        orc.close()


def test_r7_topology_sizes_change(runtime, oracle_lib):
    """topo_dom_v / topo_count_v / topo_install: other numbers of topology keys, domains and properties"""
    a, b = ru.r7()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        move_to(ev, oracle_lib, a.cfg, b, "R7", order=("quotas",))
    finally:
        ev.close()
        orc.close()


def test_r8_staged_batch_across_a_node_reload(runtime, oracle_lib):
    """soft_union / kPodNormDyn: a batch staged before ks_load_nodes was validated and flagged against the old nodes;
    ks_schedule_staged refuses it (KS_ESTATE) until it is staged again"""
    a, b = ru.r8()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        ev.stage(b.pods)
        ev.load_nodes(b.nodes.copy())
        with pytest.raises(runtime.KsError) as e:
            ev.schedule_staged()
        assert e.value.rc == abi.KS_ESTATE and "ks_stage_pods" in str(e.value)
        ob = fresh(oracle_lib, a.cfg, b)

        def staged(pods):
            ev.stage(pods)
            ev.schedule_staged()
            return ev.fetch()

        same_as_fresh(ev, ob, b.pods, {}, "R8", schedule=staged)
        ob.close()
    finally:
        ev.close()
        orc.close()


def test_r9_virtual_shards_and_pipelined_passes_survive(runtime, oracle_lib):
    """the shard setup and the pipeline mode are kept by ks_load_nodes; the chunk ranges, the gather buffer and the
    pipeline's events follow the node count (300 -> 700 nodes, 4 virtual shards, pipelined passes forced on)"""
    a, b = ru.r9()

    def setup(ev):
        ev.shard(1, 0, None, virtual_shards=4)
        ev.set_pipeline(2)

    ev, orc = start_on(runtime, oracle_lib, a, setup)
    try:
        assert ev.stats()["pipelined"] != 0
        move_to(ev, oracle_lib, a.cfg, b, "R9", order=("quotas",))
        assert ev.stats()["pipelined"] != 0
    finally:
        ev.close()
        orc.close()


def test_r10_checkpoint_across_a_node_reload(runtime, oracle_lib):
    """ckpt_blob: ks_restore after ks_load_nodes is KS_ESTATE until the next ks_checkpoint; the quota table and its
    usage survive the reload, and a checkpoint taken after it restores both"""
    a, b = ru.r10()
    ev = runtime.Evaluator(a.cfg, a.nodes.copy(), **a.tables())
    orc = fresh(oracle_lib, a.cfg, a)
    try:
        ev.checkpoint()
        half = ru.first_half(a)
        assert_same_results(ev.schedule(half), orc.schedule(half), "R10 A")
        kept = ru.keep_quotas(a.quotas, orc)
        ev.load_nodes(b.nodes.copy())
        with pytest.raises(runtime.KsError) as e:
            ev.restore()
        assert e.value.rc == abi.KS_ESTATE
        ev.checkpoint()
        ev.schedule(ru.first_half(b))
        ev.restore()
        ob = fresh(oracle_lib, a.cfg, b, quotas=kept)
        same_as_fresh(ev, ob, b.pods, {"quotas": kept}, "R10")
        ob.close()
    finally:
        ev.close()
        orc.close()


@pytest.fixture(scope="module")
def committed(oracle_lib):
    """the single-table workload, the oracle's state after the 150 commits folded into tables, and the second tables"""
    w, first, rest, other = ru.single_table()
    orc = fresh(oracle_lib, w.cfg, w)
    want = orc.schedule(first)
    f = ru.fold(w, orc)
    orc.close()
    return w, first, rest, want, f, ru.second_tables(w, other)


@pytest.mark.parametrize("table", ["quotas", "reservations", "devices", "cpu_state", "numa_nodes", "no_reservations"])
def test_single_table_reload(runtime, oracle_lib, committed, table):
    """ks_load_X on a live context with 150 commits replaces table X whole and nothing else: the context equals a
    fresh oracle on the tables as they stand (the commits folded in, X from the new table).  no_reservations: a
    zero-row table after reservations that held devices leaves no node held."""
    w, first, rest, want, f, second = committed
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    try:
        assert_same_results(ev.schedule(first), want, "first 150")
        if table == "no_reservations":
            from koordinator_amd.cluster import ReservationTable
            over = {"reservations": ReservationTable(0)}
        else:
            over = {table: second[table]}
        (k, v), = over.items()
        getattr(ev, LOADERS[k])(v.copy())
        orc = fresh(oracle_lib, w.cfg, f, **over)
        try:
            got = same_as_fresh(ev, orc, rest, tables_of(f, **over), f"reload {table}")
        finally:
            orc.close()
        if table == "no_reservations":
            assert (got["reservation"] == -1).all()
    finally:
        ev.close()


def read_backs(ev):
    """every table's read-back, by name"""
    out = {f"nodes.{k}": v.copy() for k, v in ev.read_nodes().as_dict().items()}
    out["quota used"] = ev.read_quota_used().copy()
    for k, v in zip(("used_core", "used_memory", "used_ratio", "used_rdma"), ev.read_devices()):
        out[f"devices.{k}"] = v.copy()
    for k, v in zip(("allocated", "assigned"), ev.read_reservations()):
        out[f"reservations.{k}"] = v.copy()
    out["reservations.devices"] = ev.read_reservation_devices().copy()
    for k, v in zip(("allocated", "excl_pcpu", "excl_numa"), ev.read_cpu_state()):
        out[f"cpu_state.{k}"] = v.copy()
    for k, v in zip(("used_cpu", "used_memory"), ev.read_numa_nodes()):
        out[f"numa_nodes.{k}"] = v.copy()
    return out


def assume_a_device_pod(ev, pods):
    """ks_assume of the first device pod of `pods` that still fits somewhere: (its node, the pod)"""
    from test_gpu_assume import pick

    for i in np.flatnonzero((pods.gpu_core > 0) | (pods.gpu_memory_ratio > 0)):
        pod = pods.rows([int(i)])
        node = pick(ev.eval_pod(pod)[2])
        if node < 0:
            continue
        r, _, _ = ev.assume(pod, node)
        assert r[0]["status"] == abi.KS_S_SCHEDULED and (r[0]["gpu_minors"] != 0 or r[0]["rdma_minors"] != 0)
        return node
    raise AssertionError("no device pod fits any node")


def test_restore_returns_every_table_at_once(runtime, oracle_lib, committed):
    """ks_restore brings back nodes, quotas, devices, reservations with their devices, CPU state and NUMA nodes
    together, and the host's record of assumed device pods: after a checkpoint, 300 more commits and a ks_assume,
    every read-back equals the one taken before the checkpoint, the context equals a fresh oracle on the tables as
    they stood then, and all of it a second time (a restore does not use the checkpoint up).
    test_context_reuse_premises.py::test_restore_of_every_table_premise shows that the commits reach every table."""
    from test_gpu_deltas import dev_rows

    w, first, rest, _, f, _ = committed
    t = tables_of(w)
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    orc = fresh(oracle_lib, w.cfg, w)
    try:
        assert_same_results(ev.schedule(first), orc.schedule(first), "first 150")
        same_tables(ev, orc, t, "first 150")
        before = read_backs(ev)
        for rnd in ("first restore", "second restore"):
            if rnd == "second restore":  # the context is past `rest` again: the first checkpoint still holds
                ev.restore()
                for k, v in read_backs(ev).items():
                    assert np.array_equal(v, before[k]), f"restore from the used checkpoint: {k}"
            ev.checkpoint()
            ev.schedule(rest)
            node = assume_a_device_pod(ev, w.pods)
            idx = np.array([node], np.int32)
            with pytest.raises(runtime.KsError):  # (the node holds an assumed device pod)
                ev.update_devices(idx, dev_rows(f.devices, idx))
            ev.restore()
            for k, v in read_backs(ev).items():
                assert np.array_equal(v, before[k]), f"{rnd}: {k}"
            ev.update_devices(idx, dev_rows(f.devices, idx))  # the rows it has: accepted, the assumed pod is forgotten
            of = fresh(oracle_lib, w.cfg, f)
            try:
                same_as_fresh(ev, of, rest, tables_of(f), rnd)
            finally:
                of.close()
    finally:
        ev.close()
        orc.close()


def test_dependent_tables_load_in_any_order(runtime, oracle_lib):
    """after ks_load_nodes the reservation, device, CPU-state and NUMA-node tables may be loaded in any order: all 24
    orders, one context each, against one oracle run (and hence each other)"""
    w = ru.load_order()
    orc = fresh(oracle_lib, w.cfg, w)
    want = orc.schedule(w.pods)
    t = w.tables()
    try:
        for order in ru.LOAD_ORDERS:
            label = "order " + " > ".join(order)
            ev = runtime.Evaluator(w.cfg)
            try:
                ev.load_nodes(w.nodes.copy())
                load_tables(ev, w, order=order)
                got = ev.schedule(w.pods)
                assert_same_results(got, want, label)
                for k in ("reservation", "gpu_minors", "rdma_minors"):
                    assert np.array_equal(got[k], want[k]), f"{label}: {k}"
                same_tables(ev, orc, t, label, w.pods.n)
            finally:
                ev.close()
    finally:
        orc.close()


def test_refused_load_leaves_a_usable_context(runtime, oracle_lib):
    """a NUMA table with 8-NUMA policy nodes next to reservations holding devices is refused (KS_EUNSUPPORTED) on a
    live, working context; the context then takes another cluster and equals the oracle"""
    a, wide_numa, _, b = ru.refused()
    ev, orc = start_on(runtime, oracle_lib, a)
    try:
        with pytest.raises(runtime.KsError) as e:
            ev.load_numa_nodes(wide_numa.copy())
        assert e.value.rc == abi.KS_EUNSUPPORTED and "reservations holding devices" in str(e.value)
        move_to(ev, oracle_lib, a.cfg, b, "after the refusal")
    finally:
        ev.close()
        orc.close()
