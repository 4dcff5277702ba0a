"""Scenario builders for the context-reuse tests (host-side only): a context built on workload A is moved to
workload B without closing it (test_gpu_context_reuse.py); test_context_reuse_premises.py checks on the CPU oracle
alone that each scenario reaches what it is meant to reach.  Everything is deterministic (fixed seeds)."""
from __future__ import annotations

import itertools

import numpy as np

from koordinator_amd import abi, synth
from koordinator_amd.cluster import NumaNodes

POLICY_MASK = np.uint32(3 << abi.KS_NUMA_POLICY_SHIFT)
DEPENDENT = ("reservations", "devices", "cpu_state", "numa_nodes")
LOAD_ORDERS = list(itertools.permutations(DEPENDENT))


def policy_of(nodes):
    return (nodes.numa_flags >> abi.KS_NUMA_POLICY_SHIFT) & 3


def first_half(w):
    """the pods a scenario commits on A before it moves on"""
    return w.pods.rows(np.arange(w.pods.n // 2))


def held_nodes(w) -> np.ndarray:
    """nodes with a reservation that holds devices"""
    rs = w.reservations
    if rs is None or rs.dev_allocatable is None:
        return np.zeros(0, np.int64)
    return np.unique(rs.node[(rs.dev_allocatable != 0).any(axis=1)])


def device_rows(w) -> np.ndarray:
    rs = w.reservations
    return np.flatnonzero((rs.dev_allocatable != 0).any(axis=1))


def add_policy(w, idx, policy=abi.KS_NUMA_POLICY_SINGLE_NUMA_NODE):
    """a NUMA topology policy on nodes idx (each with a CPU topology): two NUMA nodes splitting cpu and memory, the
    one-NUMA-node-per-socket CPU layout, the allocated cpuset CPUs counted per NUMA node (synth.policy_numa_nodes)"""
    nodes, cpus = w.nodes, w.cpus
    if w.numa_nodes is None:
        w.numa_nodes = NumaNodes(nodes.n)
    nn = w.numa_nodes
    nk = len(synth.CPU_TOPOLOGIES)
    W = abi.KS_CPU_WORDS
    for i in idx:
        ti = int(cpus.topology[i])
        assert ti >= 0
        if ti < nk:
            cpus.topology[i] = ti + nk
        c = int(cpus.topologies[int(cpus.topology[i])].ncpus)
        nodes.numa_flags[i] = (nodes.numa_flags[i] & ~POLICY_MASK) | np.uint32(policy << abi.KS_NUMA_POLICY_SHIFT)
        nn.count[i] = 2
        nn.alloc_cpu[i, :] = 0
        nn.alloc_memory[i, :] = 0
        nn.alloc_cpu[i, :2] = c * 1000 // 2
        nn.alloc_memory[i, :2] = int(nodes.alloc_memory[i]) // 2
        held = np.flatnonzero(np.unpackbits(cpus.allocated[i].view(np.uint8), bitorder="little")[: W * 64])
        for k in range(2):
            nn.cpuset_cpus[i, k] = int(np.count_nonzero(held // (c // 2) == k))
            nn.used_cpu[i, k] = int(nn.cpuset_cpus[i, k]) * 1000
            nn.used_memory[i, k] = 0
            nn.used_present[i, k] = 1 if nn.used_cpu[i, k] else 0
    return w


def r1():
    """A: device-holding reservations.  B: the same nodes, a NUMA policy on formerly held nodes, devices and NUMA
    table reloaded, reservations not."""
    a = synth.c3_rsv(seed=9101, n_nodes=300, n_pods=400, dev_rsv_frac=0.7)
    b = synth.c3_rsv(seed=9101, n_nodes=300, n_pods=400, dev_rsv_frac=0.7)
    held = held_nodes(a)
    turned = held[b.cpus.topology[held] >= 0]
    add_policy(b, turned)
    b.reservations = None
    return a, b, turned


def r2():
    a = synth.c4(seed=9102, n_nodes=150, n_reservations=400, n_pods=300)
    b = synth.c4(seed=9103, n_nodes=600, n_reservations=1500, n_pods=400)
    return a, b


def r3():
    """A: half of the policy nodes are device-less hosts with 4 NUMA nodes.  B: more nodes, no policy node, every
    PCIe switch on NUMA node 2 or 3."""
    a = synth.c3(seed=9104, n_nodes=200, n_pods=300)
    rng = np.random.Generator(np.random.PCG64(9105))
    pol = np.flatnonzero(policy_of(a.nodes) > 0)
    four = pol[rng.random(pol.size) < 0.5]
    d, nn = a.devices, a.numa_nodes
    for i in four:
        d.flags[i] = 0
        for col in ("total_core", "total_ratio", "total_memory", "used_core", "used_ratio", "used_memory", "total_rdma",
                    "used_rdma"):
            getattr(d, col)[:, i] = 0
        cpu, mem = int(nn.alloc_cpu[i, :2].sum()), int(nn.alloc_memory[i, :2].sum())
        nn.count[i] = 4
        nn.alloc_cpu[i, :4] = cpu // 4
        nn.alloc_memory[i, :4] = mem // 4
    b = synth.c3(seed=9106, n_nodes=500, n_pods=300, policy_frac=0.0)
    for p in range(4):
        b.devices.pcie_numa[p] = 2 + p // 2
    return a, b, four


def r4():
    """A: policy nodes with 8 NUMA nodes (the wide kernels).  B: no policy node, reservations holding devices."""
    nodes_a = 200
    a = synth.c3_rsv(seed=9107, n_nodes=nodes_a, n_pods=300)
    rng = np.random.Generator(np.random.PCG64(9108))
    nodes, nn, d = a.nodes, a.numa_nodes, a.devices
    pol = np.flatnonzero(policy_of(nodes) > 0)
    wide = pol[rng.random(pol.size) < 0.5]
    for i in wide:  # CPU-only hosts with 8 NUMA nodes (the CPU topology keeps its NUMA ids 0 and 1)
        d.flags[i] = 0
        for col in ("total_core", "total_ratio", "total_memory", "used_core", "used_ratio", "used_memory", "total_rdma",
                    "used_rdma"):
            getattr(d, col)[:, i] = 0
        cpu, mem = int(nn.alloc_cpu[i, :2].sum()), int(nn.alloc_memory[i, :2].sum())
        nn.count[i] = 8
        nn.alloc_cpu[i, :] = cpu // 8
        nn.alloc_memory[i, :] = mem // 8
    b = synth.c3_rsv(seed=9109, n_nodes=300, n_pods=500, policy_frac=0.0, dev_rsv_frac=0.7)
    return a, b, wide


def r5():
    return (synth.c2(seed=9110, n_nodes=1000, n_pods=300), synth.c2(seed=9111, n_nodes=65, n_pods=500),
            synth.c2(seed=9112, n_nodes=1, n_pods=100))


def r6():
    """B: A's nodes again, the CPU state not loaded"""
    a = synth.c3(seed=9113, n_nodes=300, n_pods=400)
    b = synth.c3(seed=9113, n_nodes=300, n_pods=400)
    b.cpus = None
    return a, b


def r7():
    a = synth.with_topology(synth.c2_default(seed=9114, n_nodes=300, n_pods=300))
    b = synth.with_topology(synth.c2_default(seed=9115, n_nodes=400, n_pods=300), seed=9116, n_zones=3, n_apps=6,
                            extra_keys={"rack": 11}, breadth_frac=0.15)
    return a, b


def r8():
    """B: A's nodes with other labels and taints (so another union of PreferNoSchedule taints)"""
    a = synth.with_static_plugins(synth.c1(seed=9117, n_nodes=300, n_pods=300), seed=9118)
    b = synth.with_static_plugins(synth.c1(seed=9117, n_nodes=300, n_pods=300), seed=9119)
    return a, b


def soft_dyn(nodes, pods) -> np.ndarray:
    """per pod: some PreferNoSchedule taint of the cluster is not tolerated (the TaintToleration score varies)"""
    union = np.bitwise_or.reduce(np.asarray(nodes.taints_soft, np.uint64)) if nodes.n else np.uint64(0)
    return (union & ~np.asarray(pods.tolerated, np.uint64)) != 0


def r9():
    return synth.c2(seed=9120, n_nodes=300, n_pods=300), synth.c2(seed=9121, n_nodes=700, n_pods=400)


def r10():
    return synth.c2(seed=9122, n_nodes=300, n_pods=300), synth.c2(seed=9123, n_nodes=400, n_pods=300)


def keep_quotas(quotas, orc):
    """the quota table a context keeps across ks_load_nodes: the loaded one with the oracle's used after the commits
    (no pod of these workloads is non-preemptible, so nonpreemptible_used stands)"""
    q = quotas.copy()
    q.used = np.ascontiguousarray(orc.read_quota_used().T)
    return q


def single_table():
    """c3_rsv with device-holding reservations; the pods committed first carry no cpuset request, so that the state
    after them can be written back into tables exactly (fold)"""
    w = add_quotas(synth.c3_rsv(seed=9124, n_nodes=300, n_pods=600, dev_rsv_frac=0.5), 32, 9130)
    plain = np.flatnonzero((w.pods.flags & abi.KS_POD_CPU_BIND) == 0)
    first = w.pods.rows(plain[:150])
    rest = w.pods.rows(np.setdiff1d(np.arange(w.pods.n), plain[:150])[:300])
    other = add_quotas(synth.c3_rsv(seed=9125, n_nodes=300, n_pods=8, dev_rsv_frac=0.5), 32, 9130)
    return w, first, rest, other


def add_quotas(w, n_quotas, seed):
    """ElasticQuota on a workload without it (as synth.c3_full does): every pod in one of n_quotas leaf quotas"""
    from koordinator_amd.config import ElasticQuotaArgs
    rng = np.random.Generator(np.random.PCG64(seed))
    p = w.pods
    batch = (p.flags & abi.KS_POD_PROD) == 0
    p.quota[:] = rng.integers(0, n_quotas, p.n)
    p.quota_req[synth.QDIM_CPU] = p.req_milli_cpu
    p.quota_req[synth.QDIM_MEMORY] = p.req_memory
    p.quota_req[synth.QDIM_BATCH_CPU] = p.req_scalar[synth.SLOT_BATCH_CPU]
    p.quota_req[synth.QDIM_BATCH_MEMORY] = p.req_scalar[synth.SLOT_BATCH_MEMORY]
    p.quota_mask[:] = np.where(batch, (1 << synth.QDIM_BATCH_CPU) | (1 << synth.QDIM_BATCH_MEMORY),
                               (1 << synth.QDIM_CPU) | (1 << synth.QDIM_MEMORY)).astype(np.uint32)
    w.quotas = synth.make_quotas(p, n_quotas, rng)
    w.profile.quota = ElasticQuotaArgs()
    return w


def fold(w, orc):
    """w's tables as they stand after the oracle's commits: node state, device usage, CPU sets, NUMA allocations and
    the reservations' allocated / assigned (the commits must not include cpuset pods: the cpuset counts of the node
    and NUMA tables have no read-back)"""
    import copy
    f = copy.copy(w)
    f.nodes = w.nodes.copy()
    for k, v in orc.read_nodes().as_dict().items():
        if k != "topo_count" or v.size:
            setattr(f.nodes, k, v.copy())
    if w.devices is not None:
        f.devices = w.devices.copy()
        f.devices.used_core, f.devices.used_memory, f.devices.used_ratio, f.devices.used_rdma = \
            [np.ascontiguousarray(x) for x in orc.read_devices()]
    if w.cpus is not None:
        f.cpus = w.cpus.copy()
        f.cpus.allocated, f.cpus.excl_pcpu, f.cpus.excl_numa = [x.copy() for x in orc.read_cpu_state()]
    if w.numa_nodes is not None:
        f.numa_nodes = w.numa_nodes.copy()
        uc, um = orc.read_numa_nodes()
        f.numa_nodes.used_cpu, f.numa_nodes.used_memory = uc.copy(), um.copy()
        f.numa_nodes.used_present = (w.numa_nodes.used_present | (uc != 0) | (um != 0)).astype(np.uint8)
    if w.reservations is not None:
        f.reservations = w.reservations.copy()
        allocated, assigned = orc.read_reservations()
        f.reservations.allocated = np.ascontiguousarray(allocated.T)
        f.reservations.assigned = assigned.copy()
        if w.reservations.dev_allocatable is not None:
            f.reservations.dev_allocated = orc.read_reservation_devices().copy()
    if w.quotas is not None:
        f.quotas = keep_quotas(w.quotas, orc)
    return f


def second_tables(w, other):
    """a second, different table of each kind for w's nodes, taken from `other` (same shape, another seed); the NUMA
    table keeps w's policy nodes (the policy is a node column) with other allocations"""
    rng = np.random.Generator(np.random.PCG64(9126))
    q = synth.make_quotas(w.pods, 40, rng, admit_frac=0.5)  # more rows, tighter limits
    nn = w.numa_nodes.copy()
    pol = policy_of(w.nodes) > 0
    for i in np.flatnonzero(pol):
        for k in range(int(nn.count[i])):
            extra = int(nn.alloc_cpu[i, k] * rng.random() * 0.3) // 1000 * 1000
            nn.used_cpu[i, k] = int(nn.cpuset_cpus[i, k]) * 1000 + extra
            nn.used_memory[i, k] = int(nn.alloc_memory[i, k] * rng.random() * 0.3) // synth.MI * synth.MI
            nn.used_present[i, k] = 1 if (nn.used_cpu[i, k] or nn.used_memory[i, k]) else 0
    # other's reservations on w's nodes: those holding devices only where w has devices and no policy
    rs = other.reservations.copy()
    bad = np.isin(rs.node, np.flatnonzero(pol | ((w.devices.flags & abi.KS_DEV_PRESENT) == 0)))
    rs.dev_allocatable[bad] = 0
    rs.dev_allocated[bad] = 0
    dv = w.devices.copy()
    used = (dv.total_ratio > 0) & (rng.random(dv.total_ratio.shape) < 0.2)
    dv.used_core = np.where(used, 100, dv.used_core)
    dv.used_ratio = np.where(used, 100, dv.used_ratio)
    dv.used_memory = np.where(used, dv.total_memory, dv.used_memory)
    cs = w.cpus.copy()
    drop = rng.random(cs.n) < 0.5  # half of the nodes with nothing allocated
    for k in ("allocated", "excl_pcpu", "excl_numa"):
        getattr(cs, k)[drop] = 0
    return {"quotas": q, "reservations": rs, "devices": dv, "cpu_state": cs, "numa_nodes": nn}


def load_order():
    return synth.c3_rsv(seed=9127, n_nodes=200, n_pods=300, dev_rsv_frac=0.5)


def refused():
    """narrow: works.  wide_numa: the same nodes' NUMA table with 8 NUMA nodes on CPU-only policy nodes, refused next
    to reservations holding devices.  b: a valid cluster to go on with."""
    a = synth.c3_rsv(seed=9128, n_nodes=150, n_pods=200, dev_rsv_frac=0.5)
    wide_numa = a.numa_nodes.copy()
    pol = np.flatnonzero((policy_of(a.nodes) > 0) & ((a.devices.flags & abi.KS_DEV_PRESENT) == 0))
    for i in pol:
        cpu, mem = int(wide_numa.alloc_cpu[i, :2].sum()), int(wide_numa.alloc_memory[i, :2].sum())
        wide_numa.count[i] = 8
        wide_numa.alloc_cpu[i, :] = cpu // 8
        wide_numa.alloc_memory[i, :] = mem // 8
    b = synth.c3_rsv(seed=9129, n_nodes=260, n_pods=300, dev_rsv_frac=0.5)
    return a, wide_numa, pol, b
