"""Nominated pods on the device (ks_load_nominated / ks_delete_nominated, ks_eval_pod_nominated,
ks_eval_pod_summary_nominated, ks_preempt_nominated; koordinator_amd/csrc/ks_nominated.h) against the reference composed
from the unchanged CPU oracle (tests/nominated_ref.py, pinned by tests/test_nominated_ref.py).  Every comparison is
exact: reasons, per-plugin scores, totals, the feasible count, the winner, the FitError counts, the top rows; for
preemption status, node, victims in order, violations and every node's dry-run outcome.

130 nodes = two full 64-node chunks and a partial one.  Entries sit on nodes 0, 63, 64 and 129, on a node with 70
entries (more than a wave's lanes), on a node whose entries are all below the pod's priority and on a node that holds
only the pod's own entry."""
import ctypes as C

import numpy as np
import pytest

import nominated_ref as ref
from koordinator_amd import abi, synth
from koordinator_amd.cluster import NominatedTable

pytestmark = pytest.mark.gpu

N = 130
PRIO = 1000       # the evaluated pod's priority
SELF = 900        # ... and its own id in the table
FIT_BITS = (abi.KS_R_FIT_PODS | abi.KS_R_FIT_CPU | abi.KS_R_FIT_MEMORY | abi.KS_R_FIT_EPHEMERAL | abi.KS_R_FIT_SCALAR)
WIDE, LOW, OWN = 17, 40, 100  # the 70-entry node, the node with lower-priority entries only, the pod's own node


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # the in-tree HIP library; no fallback
    return rt


def c2(n_nodes=N, n_pods=64):
    return synth.c2(n_nodes=n_nodes, n_pods=n_pods)


def c2_static(n_nodes=N, n_pods=64):
    """C2 with BalancedAllocation, TaintToleration and NodeAffinity (no NodePorts: outside the modelled set)"""
    w = synth.c2_default(n_nodes=n_nodes, n_pods=n_pods)
    w.profile.node_ports = False
    return w


def room(nodes, i):
    return int(nodes.alloc_milli_cpu[i] - nodes.req_milli_cpu[i])


def table(nodes):
    """the nominated table of the module docstring: every big entry takes its node's whole free cpu"""
    rows = []  # (node, priority, id, cpu, memory)
    for k, i in enumerate((0, 63, 64, 129)):
        rows.append((i, PRIO + 10 * k, k, room(nodes, i), 1 << 30))  # at (k = 0) and above the pod's priority
    rows += [(WIDE, PRIO + (j % 3) * 500 - 500, 200 + j, 250 + j, 64 << 20) for j in range(70)]  # below / at / above
    rows += [(LOW, PRIO - 1 - j, 300 + j, room(nodes, LOW), 1 << 30) for j in range(3)]
    rows.append((OWN, PRIO + 50, SELF, room(nodes, OWN), 1 << 30))
    rows.append((5, PRIO, 400, 0, 0))  # a request-less entry: only the pod count goes up
    t = NominatedTable(len(rows))
    for r, (node, prio, uid, cpu, mem) in enumerate(rows):
        t.node[r], t.priority[r], t.id[r] = node, prio, uid
        t.req[0, r], t.req[1, r] = cpu, mem
    t.req[3 + synth.SLOT_BATCH_CPU] = np.where(t.node == WIDE, 100, 0)
    return t


def a_pod(oracle_lib, w, fits_on):
    """a prod pod of the workload that the oracle finds feasible on every node of fits_on without nominated pods; with
    TaintToleration / NodeAffinity scoring, one whose normalized scores differ between nodes"""
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        first = None
        for i in np.flatnonzero((w.pods.flags & abi.KS_POD_PROD) != 0):
            pod = w.pods.rows([int(i)])
            r, s, _ = orc.eval_pod(pod)
            if r[list(fits_on)].any():
                continue
            first = pod if first is None else first
            if not w.cfg.taint.enable_score or len(np.unique(s[r == 0][:, abi.KS_SCORE_TAINT])) > 1:
                return pod
        if first is not None:
            return first
    finally:
        orc.close()
    raise AssertionError("no pod of the workload fits the chosen nodes")


def unpack(bits, n):
    flat = np.unpackbits(np.asarray(bits, np.uint64).view(np.uint8), bitorder="little")
    assert not flat[n:].any(), "padding bits set"
    return flat[:n].astype(bool)


def check_eval(ev, want, pod, label, **who):
    who = {"priority": PRIO, "self_id": SELF, **who}
    r, s, t = ev.eval_pod_nominated(pod, **who)
    assert np.array_equal(r, want["reasons"]), f"{label}: reasons differ at nodes {np.flatnonzero(r != want['reasons'])}"
    assert np.array_equal(s, want["scores"]), f"{label}: per-plugin scores"
    assert np.array_equal(t, want["total"]), f"{label}: totals"


def check_summary(ev, want, pod, label, top_n=8, mask=abi.KS_R_FIT_CPU | abi.KS_R_LA_CPU, **who):
    ws = ref.summary(want, top_n, mask)
    got = ev.eval_pod_summary_nominated(pod, top_n=top_n, unresolvable_mask=mask, want_bits=True, **who)
    n = ws["nodes"]
    for k in ("nodes", "feasible", "unresolvable", "best_node", "best_total"):
        assert got[k] == ws[k], f"{label}: {k} {got[k]} != {ws[k]}"
    assert np.array_equal(got["reason_nodes"], ws["reason_nodes"]), f"{label}: reason_nodes"
    assert np.array_equal(got["top_nodes"], ws["top_nodes"]), f"{label}: top_nodes"
    assert np.array_equal(got["top_totals"], ws["top_totals"]), f"{label}: top_totals"
    assert np.array_equal(got["top_scores"], ws["top_scores"]), f"{label}: top_scores"
    assert np.array_equal(unpack(got["feasible_bits"], n), ws["feasible_mask"]), f"{label}: feasible_bits"
    assert np.array_equal(unpack(got["unresolvable_bits"], n), ws["unresolvable_mask"]), f"{label}: unresolvable_bits"
    return got


@pytest.mark.parametrize("make", [c2, c2_static], ids=["c2", "c2-taint-affinity"])
def test_eval_and_summary_against_the_composed_reference(runtime, oracle_lib, make):
    w = make()
    nom = table(w.nodes)
    pod = a_pod(oracle_lib, w, (0, 63, 64, 129, LOW, OWN))
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ev.load_nominated(nom)
        who = dict(priority=PRIO, self_id=SELF)
        want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
        # the premises of the case: the four big entries take their nodes away, the lower-priority entries and the
        # pod's own entry do not, and nothing but Fit's bits tells pass 1 from pass 2
        for i in (0, 63, 64, 129):
            assert want["pass2"][i] == 0 and want["reasons"][i] & abi.KS_R_FIT_CPU, i
        assert want["reasons"][LOW] == 0 and want["reasons"][OWN] == 0
        assert not ((want["pass1"] ^ want["pass2"]) & ~np.uint32(FIT_BITS)).any()
        assert (want["reasons"] == 0).sum() >= 8
        check_eval(ev, want, pod, "self")
        for top_n in (0, 1, 8, 64):
            check_summary(ev, want, pod, f"self top {top_n}", top_n=top_n, **who)
        # the same pod without an entry of its own: its node's entry counts now
        who = dict(priority=PRIO, self_id=-1)
        want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
        assert want["reasons"][OWN] & abi.KS_R_FIT_CPU
        check_eval(ev, want, pod, "no self", **who)
        check_summary(ev, want, pod, "no self", **who)
        # a pod above every entry sees none; one below every entry sees them all (the 70-entry node in full)
        for prio in (PRIO + 5000, PRIO - 5000, PRIO + 500):
            who = dict(priority=prio, self_id=-1)
            want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
            check_eval(ev, want, pod, f"priority {prio}", **who)
            check_summary(ev, want, pod, f"priority {prio}", **who)
    finally:
        ev.close()


def test_seventy_entries_on_one_node_are_all_summed(runtime, oracle_lib):
    """the node's free cpu is exactly what its 70 entries and the pod need: one entry dropped or counted twice by the
    strided sum flips the verdict either way"""
    w = c2()
    nom = table(w.nodes)
    pod = a_pod(oracle_lib, w, (WIDE,))
    need = int(nom.req[0][nom.node == WIDE].sum()) + int(pod.req_milli_cpu[0])
    ev = None
    try:
        for slack, fits in ((0, True), (-1, False)):
            nodes = w.nodes.copy()
            nodes.alloc_milli_cpu[WIDE] = nodes.req_milli_cpu[WIDE] + need + slack
            nodes.la_thr_cpu[WIDE] = 0  # (LoadAware's usage check off on this node: only Fit decides)
            nodes.la_thr_memory[WIDE] = 0
            ev = runtime.Evaluator(w.cfg, nodes.copy(), **w.tables())
            ev.load_nominated(nom)
            who = dict(priority=PRIO - 5000, self_id=-1)
            want = ref.evaluate(oracle_lib, w.cfg, nodes, w.tables(), nom, pod, **who)
            assert (want["reasons"][WIDE] & abi.KS_R_FIT_CPU == 0) == fits
            check_eval(ev, want, pod, f"slack {slack}", **who)
            ev.close()
            ev = None
    finally:
        if ev is not None:
            ev.close()


@pytest.mark.parametrize("make", [c2, c2_static], ids=["c2", "c2-taint-affinity"])
def test_nominated_node_first(runtime, oracle_lib, make):
    w = make()
    nom = table(w.nodes)
    pod = a_pod(oracle_lib, w, (0, 63, 64, 129, LOW, OWN))
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ev.load_nominated(nom)
        # the pod's nominated node is the one that holds its own entry: feasible, so it is the whole result
        who = dict(priority=PRIO, self_id=SELF, nominated_node=OWN)
        want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
        assert want["single"] == OWN
        got = check_summary(ev, want, pod, "feasible nominated node", **who)
        assert got["feasible"] == 1 and got["best_node"] == OWN and list(got["top_nodes"]) == [OWN]
        # ks_eval_pod_nominated keeps every node's own reasons and scores (no KS_R_* bit is free to mark the others)
        full = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, priority=PRIO, self_id=SELF)
        check_eval(ev, full, pod, "eval_pod_nominated with a nominated node", **who)
        # nominated to node 63, which fails only because of the higher-priority nominated pod there: the full sweep
        who = dict(priority=PRIO, self_id=SELF, nominated_node=63)
        want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
        assert want["single"] == -1 and want["pass2"][63] == 0 and want["reasons"][63] != 0
        got = check_summary(ev, want, pod, "infeasible nominated node", **who)
        assert got["feasible"] > 1
    finally:
        ev.close()


def after(w, orc):
    """the workload's node and quota tables as the oracle holds them after its assumes"""
    st = orc.read_nodes().as_dict()
    nodes = w.nodes.copy()
    for k, v in st.items():
        if k not in ("host_ports", "topo_count"):
            getattr(nodes, k)[...] = v
    q = w.quotas.copy()
    q.used[:] = orc.read_quota_used().T
    return nodes, {"quotas": q}


@pytest.mark.parametrize("restore", [False, True], ids=["plain", "checkpoint-restore"])
def test_assume_then_delete_sequence(runtime, oracle_lib, restore):
    """the shim's cycle: the nominated pod of node 63 is assumed there and leaves the table; the other pod is refused
    the room before (nominated) and after (Requested), and node 63's other entries keep counting"""
    w = c2()
    nom = table(w.nodes)
    pod = a_pod(oracle_lib, w, (0, 63, 64, 129, LOW, OWN))
    mover = pod.rows([0])  # the nominated pod of node 63 as a pod: the entry's requests
    row = int(np.flatnonzero(nom.id == 1)[0])
    assert nom.node[row] == 63
    mover.req_milli_cpu[0] = mover.nonzero_milli_cpu[0] = mover.la_req_cpu[0] = nom.req[0, row]
    mover.req_memory[0] = mover.nonzero_memory[0] = mover.la_req_memory[0] = nom.req[1, row]
    mover.quota_req[synth.QDIM_CPU, 0], mover.quota_req[synth.QDIM_MEMORY, 0] = nom.req[0, row], nom.req[1, row]
    mover.flags[0] &= ~np.uint32(abi.KS_POD_NONPREEMPTIBLE)
    who = dict(priority=PRIO, self_id=SELF)
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ev.load_nominated(nom)
        if restore:
            ev.checkpoint()
        rounds = 2 if restore else 1
        for rnd in range(rounds):
            want = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, pod, **who)
            check_eval(ev, want, pod, f"round {rnd} before")
            check_summary(ev, want, pod, f"round {rnd} before", **who)
            ev.assume(mover, 63)
            ev.delete_nominated([1])
            if rnd == 0:
                orc.assume(mover, 63)
            nodes2, tables2 = after(w, orc)
            nom2 = nom.rows(np.flatnonzero(nom.id != 1))
            want2 = ref.evaluate(oracle_lib, w.cfg, nodes2, tables2, nom2, pod, **who)
            assert want2["pass2"][63] & abi.KS_R_FIT_CPU  # the room is taken for good now
            check_eval(ev, want2, pod, f"round {rnd} after")
            check_summary(ev, want2, pod, f"round {rnd} after", **who)
            if restore:
                ev.restore()  # back to the checkpoint: the node columns and the table with id 1 in it
    finally:
        ev.close()
        orc.close()


PKEYS = ("status", "node", "num_pdb_violations", "candidates", "potential_nodes")


def test_preempt_against_the_composed_reference(runtime, oracle_lib):
    """synth.c2_preempt(n_nodes=100) with one node of more than 64 pods (the dry run's multi-slot path); nominated
    entries at, above and below the preemptor's priority on nodes that are candidates without them, one the
    preemptor's own"""
    w = synth.c2_preempt(n_nodes=100, n_preemptors=12)
    nodes, t = w.nodes, w.node_pods
    # node 7 gets 70 more running pods: copies of its own, later start times, requests added to its NodeInfo
    own = np.flatnonzero(t.node == 7)
    extra = t.rows(np.resize(own, 70))
    extra.start_time[:] = t.start_time.max() + 1 + np.arange(70)
    big = type(t)(t.m + 70, len(t.pdb_allowed))
    for k in ("node", "priority", "start_time", "flags", "quota", "pdb"):
        getattr(big, k)[:] = np.concatenate([getattr(t, k), getattr(extra, k)])
    for k in ("req", "quota_req", "pdb_more"):
        getattr(big, k)[:] = np.concatenate([getattr(t, k), getattr(extra, k)], axis=1)
    big.pdb_allowed[:] = t.pdb_allowed
    nodes.req_milli_cpu[7] += extra.req[0].sum()
    nodes.req_memory[7] += extra.req[1].sum()
    for k in range(abi.KS_MAX_SCALARS):
        nodes.req_scalar[k][7] += extra.req[3 + k].sum()
    nodes.pod_count[7] += 70
    nodes.allowed_pods[7] = 200
    nodes.alloc_milli_cpu[7] = nodes.req_milli_cpu[7] + 500
    nodes.alloc_memory[7] = nodes.req_memory[7] + (512 << 30)
    for k in range(abi.KS_MAX_SCALARS):
        nodes.alloc_scalar[k][7] = nodes.req_scalar[k][7] * 2 + 1
    quotas = w.quotas.copy()
    inq = ((extra.flags & abi.KS_NPOD_IN_QUOTA) != 0) & (extra.quota >= 0)
    for d in range(abi.KS_QUOTA_DIMS):
        np.add.at(quotas.used[d], extra.quota[inq], extra.quota_req[d][inq])
    quotas.limit[:] = np.maximum(quotas.limit, quotas.used)
    assert np.bincount(big.node, minlength=nodes.n).max() > 64

    ev = runtime.Evaluator(w.cfg, nodes.copy(), quotas.copy())
    plain = oracle_lib.Oracle(w.cfg, nodes.copy(), quotas.copy())
    try:
        ev.load_node_pods(big)
        plain.load_node_pods(big)
        nominated = changed = 0
        for i in range(w.preemptors.n):
            pod, prio = w.preemptors.rows([i]), int(w.priority[i])
            base = plain.preempt(pod, prio, node_status=True)
            cands = np.flatnonzero(base["node_status"] == abi.KS_PN_CANDIDATE)
            if len(cands) < 4:
                continue
            picks = [int(base["node"])] + [int(c) for c in cands if c != base["node"]][:3]
            if 7 in cands and 7 not in picks:
                picks[-1] = 7
            # above, at and below the preemptor's priority and one more above; then the preemptor's own entry, on the
            # node whose other entry is below its priority, so that node is lost only when the entry is not its own
            rows = list(zip(picks + [picks[2]], [prio + 100, prio, prio - 1, prio + 7, prio + 50], [50, 51, 52, 53, SELF]))
            nom = NominatedTable(len(rows))
            for r, (node, p, uid) in enumerate(rows):
                nom.node[r], nom.priority[r], nom.id[r] = node, p, uid
                nom.req[0, r], nom.req[1, r] = 1 << 40, 1 << 30  # no victim frees this much cpu
            ev.load_nominated(nom)
            for self_id in (SELF, -1):
                want = ref.preempt(oracle_lib, w.cfg, nodes, quotas, big, nom, pod, prio, self_id=self_id)
                got = ev.preempt(pod, prio, node_status=True, self_id=self_id)
                label = f"preemptor {i} self {self_id}"
                for k in PKEYS:
                    assert got[k] == want[k], f"{label}: {k} {got[k]} (GPU) vs {want[k]} (composed oracle)"
                assert np.array_equal(got["victims"], want["victims"]), f"{label}: victims"
                assert np.array_equal(got["node_status"], want["node_status"]), f"{label}: node statuses"
                if self_id == -1:  # ks_preempt itself with a table loaded is ks_preempt_nominated(self_id = -1)
                    again = ev.preempt(pod, prio, node_status=True)
                    assert again["node"] == got["node"] and np.array_equal(again["node_status"], got["node_status"])
                changed += int(not np.array_equal(want["node_status"], base["node_status"]))
                nominated += int(want["status"] == abi.KS_P_NOMINATED)
        assert changed >= 4 and nominated >= 2, (changed, nominated)  # the entries moved real outcomes
    finally:
        ev.close()
        plain.close()


def with_plugin(name):
    if name == "nodeports":
        return synth.c2_default(n_nodes=N, n_pods=8)
    if name == "topology":
        return synth.with_topology(synth.c2(n_nodes=N, n_pods=8))
    if name in ("numa", "deviceshare"):
        return synth.c3(n_nodes=N, n_pods=8)  # (both plugins: the message names every plugin outside the set)
    return synth.c4(n_nodes=N, n_reservations=40, n_pods=8)


@pytest.mark.parametrize("name", ["nodeports", "topology", "numa", "deviceshare", "reservation"])
def test_profiles_outside_the_set_refuse_a_table(runtime, name):
    w = with_plugin(name)
    cfg = w.cfg
    on = {"nodeports": cfg.nodeports.enable_filter, "topology": cfg.topology.enable, "numa": cfg.numa.enable,
          "deviceshare": cfg.deviceshare.enable, "reservation": cfg.reservation.enable}
    assert on[name], "the workload does not enable the plugin under test"
    ev = runtime.Evaluator(cfg, w.nodes.copy(), **w.tables())
    try:
        nom = NominatedTable(1)
        nom.req[0, 0] = 1000
        with pytest.raises(runtime.KsError) as e:
            ev.load_nominated(nom)
        assert e.value.rc == abi.KS_EUNSUPPORTED
        words = {"nodeports": "NodePorts", "topology": "PodTopologySpread", "numa": "NodeNUMAResource",
                 "deviceshare": "DeviceShare", "reservation": "Reservation"}
        assert words[name] in str(e.value)
        ev.load_nominated(None)  # an empty table is always accepted
        ev.eval_pod(w.pods.rows([0]))
    finally:
        ev.close()


def test_old_entry_points_refuse_while_a_table_is_loaded(runtime, oracle_lib):
    w = c2()
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ev.load_nominated(table(w.nodes))
        pod = w.pods.rows([0])
        calls = {"ks_schedule": lambda: ev.schedule(w.pods), "ks_stage_pods": lambda: ev.stage(w.pods),
                 "ks_eval_pod": lambda: ev.eval_pod(pod), "ks_eval_pod_summary": lambda: ev.eval_pod_summary(pod, top_n=4)}
        for name, call in calls.items():
            with pytest.raises(runtime.KsError) as e:
                call()
            assert e.value.rc == abi.KS_EUNSUPPORTED, name
            assert "nominated" in str(e.value), name
        # cleared: they all run again and equal the oracle
        ev.load_nominated(None)
        r, s, t = orc.eval_pod(pod)
        gr, gs, gt = ev.eval_pod(pod)
        assert np.array_equal(gr, r) and np.array_equal(gs, s) and np.array_equal(gt, t)
        got = ev.eval_pod_summary(pod, top_n=4)
        assert got["feasible"] == int((r == 0).sum())
        ev.stage(w.pods)
        ev.schedule_staged()
        staged = ev.fetch()
        want = orc.schedule(w.pods)
        for k in ("node", "status", "score"):
            assert np.array_equal(staged[k], want[k]), k
    finally:
        ev.close()
        orc.close()


def test_invalid_tables(runtime):
    w = c2()
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    try:
        good = table(w.nodes)
        for name, spoil in (("duplicate id", lambda t: t.id.__setitem__(3, t.id[2])),
                            ("node row out of range", lambda t: t.node.__setitem__(0, N)),
                            ("negative node row", lambda t: t.node.__setitem__(0, -1)),
                            ("negative request", lambda t: t.req.__setitem__((1, 4), -5))):
            bad = good.copy()
            spoil(bad)
            with pytest.raises(runtime.KsError) as e:
                ev.load_nominated(bad)
            assert e.value.rc == abi.KS_EINVAL, name
        with pytest.raises(runtime.KsError) as e:
            ev.load_nominated(good, sizeof_cols=C.sizeof(abi.KsNominatedCols) + 8)
        assert e.value.rc == abi.KS_EINVAL and "sizeof" in str(e.value)
        with pytest.raises(runtime.KsError) as e:
            ev.eval_pod_nominated(w.pods.rows([0]), priority=PRIO, nominated_node=N)
        assert e.value.rc == abi.KS_EINVAL
        ev.load_nominated(good)  # a refused load leaves a context that takes the next one
    finally:
        ev.close()


def test_load_nodes_drops_the_table(runtime, oracle_lib):
    w = c2()
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        ev.load_nominated(table(w.nodes))
        ev.load_nodes(w.nodes.copy())
        pod = w.pods.rows([0])
        r, s, t = orc.eval_pod(pod)
        gr, gs, gt = ev.eval_pod(pod)  # not refused: no table
        assert np.array_equal(gr, r) and np.array_equal(gs, s) and np.array_equal(gt, t)
    finally:
        ev.close()
        orc.close()


def test_no_table_ever_loaded(runtime, oracle_lib):
    """the NULL-pointer paths: without a table the old and the new entry points return what the oracle returns"""
    w = c2_static()
    pod = w.pods.rows([1])
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    orc = oracle_lib.Oracle(w.cfg, w.nodes.copy(), **w.tables())
    try:
        r, s, t = orc.eval_pod(pod)
        want = {"reasons": r, "scores": s, "total": t, "single": -1}
        ws = ref.summary(want, 8, abi.KS_R_FIT_CPU)
        for got in (ev.eval_pod_summary(pod, top_n=8, unresolvable_mask=abi.KS_R_FIT_CPU),
                    ev.eval_pod_summary_nominated(pod, priority=PRIO, top_n=8, unresolvable_mask=abi.KS_R_FIT_CPU)):
            for k in ("nodes", "feasible", "unresolvable", "best_node", "best_total"):
                assert got[k] == ws[k], k
            for k in ("reason_nodes", "top_nodes", "top_totals", "top_scores"):
                assert np.array_equal(got[k], ws[k]), k
        gr, gs, gt = ev.eval_pod_nominated(pod, priority=PRIO)
        assert np.array_equal(gr, r) and np.array_equal(gs, s) and np.array_equal(gt, t)
    finally:
        ev.close()
        orc.close()
    p = synth.c2_preempt(n_nodes=100, n_preemptors=6)
    ev = runtime.Evaluator(p.cfg, p.nodes.copy(), p.quotas.copy())
    orc = oracle_lib.Oracle(p.cfg, p.nodes.copy(), p.quotas.copy())
    try:
        ev.load_node_pods(p.node_pods)
        orc.load_node_pods(p.node_pods)
        for i in range(p.preemptors.n):
            pod, prio = p.preemptors.rows([i]), int(p.priority[i])
            want = orc.preempt(pod, prio, node_status=True)
            for got in (ev.preempt(pod, prio, node_status=True), ev.preempt(pod, prio, node_status=True, self_id=3)):
                for k in PKEYS:
                    assert got[k] == want[k], (i, k)
                assert np.array_equal(got["victims"], want["victims"])
                assert np.array_equal(got["node_status"], want["node_status"])
    finally:
        ev.close()
        orc.close()
