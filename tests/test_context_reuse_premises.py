"""The premises of the context-reuse scenarios (reuse_util.py), on the CPU oracle alone: each scenario's workloads
must reach what the scenario is about, or the GPU test that uses them (test_gpu_context_reuse.py) checks nothing.
A premise that fails is a broken builder."""
import numpy as np
import pytest

import reuse_util as ru
from helpers import assert_same_results, assert_same_state
from koordinator_amd import abi


def oracle_of(oracle_lib, cfg, w, **over):
    t = w.tables()
    t.update(over)
    return oracle_lib.Oracle(cfg, w.nodes.copy(), nthreads=8, **{k: v for k, v in t.items() if v is not None})


def placed(res):
    return res["status"] == abi.KS_S_SCHEDULED


def test_same_profile_for_every_step(oracle_lib):
    """a context keeps its ks_config: the workloads of a scenario must share it byte for byte"""
    for build in (ru.r1, ru.r2, ru.r3, ru.r4, ru.r5, ru.r6, ru.r7, ru.r8, ru.r9, ru.r10):
        ws = [w for w in build() if hasattr(w, "cfg")]
        for w in ws[1:]:
            assert bytes(w.cfg) == bytes(ws[0].cfg), build.__name__
    a, _, b = ru.refused()[0], None, ru.refused()[3]
    assert bytes(a.cfg) == bytes(b.cfg)
    w, _, _, other = ru.single_table()
    assert bytes(w.cfg) == bytes(other.cfg)


def test_r1_held_nodes_turn_into_policy_nodes_with_device_pods(oracle_lib):
    a, b, turned = ru.r1()
    assert a.nodes.n == b.nodes.n and b.reservations is None
    assert np.isin(turned, ru.held_nodes(a)).all()
    assert (ru.policy_of(a.nodes)[turned] == 0).all() and (ru.policy_of(b.nodes)[turned] != 0).all()
    got = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    dev = placed(got) & ((got["gpu_minors"] != 0) | (got["rdma_minors"] != 0))
    hit = np.intersect1d(turned, got["node"][dev])
    assert hit.size >= 20, hit.size
    # A's first half commits something
    assert placed(oracle_of(oracle_lib, a.cfg, a).schedule(ru.first_half(a))).sum() >= 50


def test_r2_grows_past_the_padding_with_reservation_pods(oracle_lib):
    a, b = ru.r2()
    assert b.nodes.n > (a.nodes.n + 63) // 64 * 64
    assert a.reservations.r > 0 and b.reservations.r > a.reservations.r
    got = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    assert (placed(got) & (got["reservation"] >= 0)).sum() >= 50
    got = oracle_of(oracle_lib, a.cfg, a).schedule(ru.first_half(a))
    assert (placed(got) & (got["reservation"] >= 0)).sum() >= 10


def test_r3_four_numa_rows_then_devices_on_numa_2_and_3(oracle_lib):
    a, b, four = ru.r3()
    assert four.size >= 20 and (a.numa_nodes.count[four] == 4).all() and four.max() < b.nodes.n
    assert b.nodes.n > a.nodes.n and (ru.policy_of(b.nodes) == 0).all() and b.numa_nodes is None
    assert sorted(set(np.unique(b.devices.pcie_numa[:4]))) == [2, 3]
    # rows that held a policy node in A carry devices in B (what a stale per-node NUMA count would be checked against)
    assert ((b.devices.flags[: a.nodes.n] & abi.KS_DEV_PRESENT) != 0)[ru.policy_of(a.nodes) > 0].sum() >= 20
    got = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    assert (placed(got) & (got["gpu_minors"] != 0)).sum() >= 30
    assert placed(oracle_of(oracle_lib, a.cfg, a).schedule(ru.first_half(a))).sum() >= 50


def test_r4_wide_then_device_holding_reservations(oracle_lib):
    a, b, wide = ru.r4()
    assert wide.size >= 20 and (a.numa_nodes.count[wide] == 8).all()
    assert (ru.policy_of(b.nodes) == 0).all() and b.numa_nodes is None
    got = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    rows = ru.device_rows(b)
    in_held = placed(got) & (got["gpu_minors"] != 0) & np.isin(got["reservation"], rows)
    assert in_held.sum() >= 30, int(in_held.sum())
    ga = oracle_of(oracle_lib, a.cfg, a).schedule(ru.first_half(a))
    assert (placed(ga) & np.isin(ga["node"], wide)).sum() >= 5


def test_r5_shrinks_across_the_word_and_to_one_node(oracle_lib):
    a, b, c = ru.r5()
    assert (a.nodes.n, b.nodes.n, c.nodes.n) == (1000, 65, 1)
    assert a.quotas.q == b.quotas.q == c.quotas.q
    for w in (a, b, c):
        assert not (w.pods.flags & abi.KS_POD_NONPREEMPTIBLE).any()
    oa = oracle_of(oracle_lib, a.cfg, a)
    assert placed(oa.schedule(ru.first_half(a))).sum() >= 50
    kept = ru.keep_quotas(a.quotas, oa)
    assert (kept.used != a.quotas.used).any()
    got = oracle_of(oracle_lib, a.cfg, b, quotas=kept).schedule(b.pods)
    assert placed(got).sum() >= 30 and (got["node"][placed(got)] == 64).any()


def test_r6_cpuset_pods_meet_nodes_without_cpu_state(oracle_lib):
    a, b = ru.r6()
    assert b.cpus is None and a.cpus is not None
    bind = (b.pods.flags & abi.KS_POD_CPU_BIND) != 0
    assert bind.sum() >= 50
    ga = oracle_of(oracle_lib, a.cfg, a).schedule(ru.first_half(a))
    assert (placed(ga) & bind[: len(ga["node"])]).sum() >= 20  # A commits cpusets
    gb = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    assert not (placed(gb) & bind).any() and placed(gb).sum() >= 50


def test_r7_topology_sizes_differ(oracle_lib):
    a, b = ru.r7()
    sa = (a.nodes.topo_domain.shape[0], a.nodes.topo_ndomains, a.nodes.topo_count.shape[0])
    sb = (b.nodes.topo_domain.shape[0], b.nodes.topo_ndomains, b.nodes.topo_count.shape[0])
    assert sa[0] != sb[0] and sa[1] != sb[1] and sa[2] != sb[2], (sa, sb)
    got = oracle_of(oracle_lib, a.cfg, b).schedule(b.pods)
    assert placed(got).sum() >= 50 and (~placed(got)).sum() >= 1


def test_r8_soft_taint_union_changes_the_pods_flag(oracle_lib):
    a, b = ru.r8()
    assert a.nodes.n == b.nodes.n
    ua = np.bitwise_or.reduce(a.nodes.taints_soft)
    ub = np.bitwise_or.reduce(b.nodes.taints_soft)
    assert ua != ub
    flips = ru.soft_dyn(a.nodes, b.pods) != ru.soft_dyn(b.nodes, b.pods)
    assert flips.sum() >= 10, int(flips.sum())


def test_r9_r10_sizes(oracle_lib):
    a, b = ru.r9()
    assert (a.nodes.n + 63) // 64 >= 4 and b.nodes.n > 2 * a.nodes.n
    a, b = ru.r10()
    assert a.quotas.q == b.quotas.q and not (a.pods.flags & abi.KS_POD_NONPREEMPTIBLE).any()
    oa = oracle_of(oracle_lib, a.cfg, a)
    oa.schedule(ru.first_half(a))
    assert (ru.keep_quotas(a.quotas, oa).used != a.quotas.used).any()


def test_fold_is_exact(oracle_lib):
    """the single-table scenarios compare with a fresh oracle built from the tables after 150 commits: an oracle that
    goes on from those commits and a fresh one on the folded tables must agree on everything"""
    w, first, rest, _ = ru.single_table()
    assert first.n == 150 and rest.n >= 250
    o1 = oracle_of(oracle_lib, w.cfg, w)
    g1 = o1.schedule(first)
    assert placed(g1).sum() >= 100 and (placed(g1) & (g1["reservation"] >= 0)).sum() >= 20
    assert (placed(g1) & (g1["gpu_minors"] != 0)).sum() >= 20
    f = ru.fold(w, o1)
    o2 = oracle_of(oracle_lib, w.cfg, f)
    want, got = o1.schedule(rest), o2.schedule(rest)
    assert_same_results(got, want, "fold")
    for k in ("reservation", "gpu_minors", "rdma_minors"):
        assert np.array_equal(got[k], want[k]), k
    assert_same_state(o2.read_nodes(), o1.read_nodes(), "fold")
    for rd in ("read_devices", "read_cpu_state", "read_numa_nodes", "read_reservations"):
        for x, y in zip(getattr(o2, rd)(), getattr(o1, rd)()):
            assert np.array_equal(x, y), rd
    assert np.array_equal(o2.read_reservation_devices(), o1.read_reservation_devices())


def test_restore_of_every_table_premise(oracle_lib):
    """test_restore_returns_every_table_at_once dirties every table between ks_checkpoint and ks_restore with `rest`:
    after `first`, `rest` must commit into quotas, devices (RDMA too), cpusets, a reservation that holds devices and a
    NUMA-policy node, and the workload must have device pods left to ks_assume"""
    w, first, rest, _ = ru.single_table()
    o = oracle_of(oracle_lib, w.cfg, w)
    o.schedule(first)
    before = (o.read_quota_used().copy(), [x.copy() for x in o.read_devices()], [x.copy() for x in o.read_cpu_state()],
              [x.copy() for x in o.read_numa_nodes()], [x.copy() for x in o.read_reservations()],
              o.read_reservation_devices().copy())
    got = o.schedule(rest)
    ok = placed(got)
    in_dev_rsv = ok & np.isin(got["reservation"], ru.device_rows(w)) & (got["gpu_minors"] != 0)
    assert in_dev_rsv.sum() >= 1, "no pod of rest takes devices from a reservation that holds them"
    on_policy = ok & (ru.policy_of(w.nodes)[np.where(ok, got["node"], 0)] != 0)
    assert on_policy.sum() >= 1, "no pod of rest lands on a NUMA-policy node"
    assert not np.array_equal(o.read_quota_used(), before[0])
    assert all(not np.array_equal(x, y) for x, y in zip(o.read_devices(), before[1])), "devices incl. RDMA"
    assert not np.array_equal(o.read_cpu_state()[0], before[2][0])
    assert not np.array_equal(o.read_numa_nodes()[0], before[3][0])
    assert all(not np.array_equal(x, y) for x, y in zip(o.read_reservations(), before[4]))
    assert not np.array_equal(o.read_reservation_devices(), before[5])
    assert ((rest.gpu_core > 0) | (rest.gpu_memory_ratio > 0)).sum() >= 10


def test_second_tables_differ_and_load(oracle_lib):
    w, first, rest, other = ru.single_table()
    t2 = ru.second_tables(w, other)
    assert t2["quotas"].q > w.quotas.q
    assert ru.held_nodes(w).size >= 20
    rs2 = t2["reservations"]
    assert rs2.r > 0 and not np.array_equal(rs2.node, w.reservations.node)
    assert (rs2.dev_allocatable != 0).any()
    assert not np.array_equal(t2["devices"].used_core, w.devices.used_core)
    assert not np.array_equal(t2["cpu_state"].allocated, w.cpus.allocated)
    assert not np.array_equal(t2["numa_nodes"].used_cpu, w.numa_nodes.used_cpu)
    base = oracle_of(oracle_lib, w.cfg, w).schedule(rest)
    for k, v in t2.items():
        got = oracle_of(oracle_lib, w.cfg, w, **{k: v}).schedule(rest)
        assert placed(got).sum() >= 50, k
        assert not (np.array_equal(got["node"], base["node"]) and np.array_equal(got["score"], base["score"])), k


def test_load_order_and_refused_premises(oracle_lib):
    assert len(ru.LOAD_ORDERS) == 24
    w = ru.load_order()
    assert all(t is not None for t in (w.reservations, w.devices, w.cpus, w.numa_nodes)) and ru.held_nodes(w).size >= 10
    a, wide_numa, pol, b = ru.refused()
    assert pol.size >= 3 and (wide_numa.count[pol] == 8).all() and ru.held_nodes(a).size >= 10
    assert b.nodes.n != a.nodes.n
