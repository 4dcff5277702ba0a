"""The device's score arithmetic at its numeric boundaries (ks_device.h term_least / term_most, pct_floor_i64,
small_div; the Term state of term_set, ks_fq.h build_row, the slot rows of ks_mono.h / ks_pass.h, term_take), against
the CPU oracle and the Go formulas restated in Python integers (score_edge_util.py; tests/test_score_edges.py checks
the oracle against that restatement on the same cases).  Every comparison is exact.

The cases: quotients 100 (h - p) / c on an integer or one unit (1/c) off one; capacities 1 .. 999, primes of 5, 11 and
13 digits, 3 * 2^37, 2^43 - 7 .. 2^43 + 1 (the switch between the f64 and the int64 path), 2^44 - 17 and 2^44 - 15
(where the f64 formula would be off by one), 2^47 + 12345, 2^55 + 7, 2^56 - 1 (the validated limit); pod requests
0, 1, 12345, 2^46 - 1 .. 2^46 + 1 (the pod side of the switch), 2^55; zero capacities; 64-node chunks that are all
below 2^43, all above, and alternating lane by lane.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import score_edge_util as U
from koordinator_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS_RAN = 2  # ks_stats.commit_helpers: the fq kernel's evaluator wave (slot-key table) ran


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # must load the in-tree HIP library; no fallback
    return rt


@pytest.fixture(scope="module")
def cases():
    return [U.Case(s) for s in U.matrix()]


# ---- a. ks_eval_pod on the case set ---------------------------------------------------------------------------------

def eval_three_way(runtime, oracle_lib, c):
    tag = c.spec.name()
    ev = runtime.Evaluator(c.cfg, c.nodes.copy(), **c.tables())
    orc = oracle_lib.Oracle(c.cfg, c.nodes.copy(), **c.tables())
    try:
        r_g, s_g, t_g = ev.eval_pod(c.pod)
        r_o, s_o, t_o = orc.eval_pod(c.pod)
    finally:
        ev.close()
        orc.close()
    assert not r_o.any(), f"{tag}: the oracle rejects node {int(np.nonzero(r_o)[0][0])}"
    assert np.array_equal(r_g, r_o), f"{tag}: reasons"
    for col, key in ((abi.KS_SCORE_FIT, "fit"), (abi.KS_SCORE_LOADAWARE, "la"), (abi.KS_SCORE_NUMA, "numa")):
        bad = np.nonzero(s_g[:, col] != c.want[key])[0]
        assert not len(bad), f"{tag}: {key} differs from the Go formula on {len(bad)} nodes; node {int(bad[0])}" \
                             f"{' (>= 2^43)' if U.node_is_big(int(bad[0])) else ''}: device {int(s_g[bad[0], col])}, " \
                             f"formula {int(c.want[key][bad[0]])}, terms (c, d, p) {c.used[bad[0]]}"
    assert np.array_equal(s_g, s_o), f"{tag}: score columns differ from the oracle"
    assert np.array_equal(t_g, t_o), f"{tag}: total differs from the oracle"
    assert np.array_equal(t_g, c.want["total"]), f"{tag}: total differs from the Go formula"


@pytest.mark.parametrize("part", range(4))
def test_eval_pod_on_the_case_set(runtime, oracle_lib, cases, part):
    """the whole matrix of tests/test_score_edges.py, a quarter per case (one context per evaluation case)"""
    mine = cases[part::4]
    assert mine
    for c in mine:
        eval_three_way(runtime, oracle_lib, c)


# ---- b. Reserves that walk a node's quotient across integer boundaries -------------------------------------------------

def with_env(name, value, fn):
    """KS_FQ_KEYS / KS_COMMIT_FQ are read when a context is created"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def plan_agrees(plan, st, label):
    """the context reports the LDS image and the helper count of the host's plan for the same inputs"""
    keys = plan["fq_keys"] and not plan["mono"]
    assert st["commit_lds_bytes"] == (plan["fq_smem"] if keys else plan["smem"]), f"{label}: {plan} vs {st['commit_lds_bytes']}"
    assert st["commit_helpers"] == (KEYS_RAN if keys else 0), label


def test_reserve_walk_monotone_kernel(runtime, oracle_lib):
    """Fit + LoadAware without quota: the monotone kernel's prebuilt rows (ks_mono.h)"""
    plan = U.commit_plans()["mono"]
    assert plan["mono"] and not plan["fq"], plan
    st, _ = U.run_reserve_walk(runtime, oracle_lib, quota=False, label="mono")
    print("mono stats", st["commit_helpers"], st["commit_lds_bytes"], st["passes"], plan)
    plan_agrees(plan, st, "mono")


def test_reserve_walk_fq_kernel_with_and_without_keys(runtime, oracle_lib):
    """Fit + LoadAware + ElasticQuota: the dedicated kernel (ks_fq.h), its rows built by build_row, with the slot-key
    table (the default) and with KS_FQ_KEYS=0; and KS_COMMIT_FQ=0, the general kernel with quota"""
    st_k, w_k = with_env("KS_FQ_KEYS", "1", lambda: U.run_reserve_walk(runtime, oracle_lib, quota=True, label="fq-keys"))
    st_w, w_w = with_env("KS_FQ_KEYS", "0", lambda: U.run_reserve_walk(runtime, oracle_lib, quota=True, label="fq-wave0"))
    st_g, w_g = with_env("KS_COMMIT_FQ", "0", lambda: U.run_reserve_walk(runtime, oracle_lib, quota=True, label="general-quota"))
    print("fq stats helpers", st_k["commit_helpers"], st_w["commit_helpers"], st_g["commit_helpers"], "LDS",
          st_k["commit_lds_bytes"], st_w["commit_lds_bytes"], st_g["commit_lds_bytes"])
    plans = U.commit_plans()
    assert plans["fq-keys"]["fq"] and plans["fq-keys"]["fq_keys"] and not plans["fq-keys"]["mono"], plans["fq-keys"]
    assert plans["fq-wave0"]["fq"] and not plans["fq-wave0"]["fq_keys"] and not plans["fq-wave0"]["mono"], plans["fq-wave0"]
    assert not plans["general-quota"]["fq"] and not plans["general-quota"]["mono"], plans["general-quota"]
    for name, st in (("fq-keys", st_k), ("fq-wave0", st_w), ("general-quota", st_g)):
        plan_agrees(plans[name], st, name)
    assert st_k["commit_helpers"] == KEYS_RAN, "the slot-key table did not run"
    assert st_w["commit_helpers"] == 0 and st_g["commit_helpers"] == 0
    assert st_k["commit_lds_bytes"] > st_w["commit_lds_bytes"], "the image with the table is the larger one"
    assert st_k["commit_lds_bytes"] <= 160 * 1024
    assert any((np.asarray(w["status"]) & abi.KS_S_QUOTA).any() for w in w_k), "no pod was rejected by its quota"


@pytest.mark.parametrize("kw", [dict(batch_pods=7), dict(candidates=2), dict(vshards=2)], ids=["batch7", "cand2", "vshards2"])
@pytest.mark.parametrize("quota", [False, True], ids=["noquota", "quota"])
def test_reserve_walk_pass_shapes(runtime, oracle_lib, quota, kw):
    U.run_reserve_walk(runtime, oracle_lib, quota=quota, label=f"shape-{kw}", **kw)


CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import score_edge_util as U
from koordinator_amd import runtime
from oracle import oracle
st, _ = U.run_reserve_walk(runtime, oracle, quota=os.environ["EDGE_QUOTA"] == "1", label="child")
print("EDGE OK helpers=%d lds=%d passes=%d" % (st["commit_helpers"], st["commit_lds_bytes"], st["passes"]))
"""


@pytest.mark.parametrize("mode,quota", [("1", False), ("2", True)], ids=["general-noquota", "mono-quota"])
def test_reserve_walk_forced_commit_kernel(mode, quota):
    """KS_COMMIT_GENERAL is read once per process: =1 the general kernel without quota, =2 the monotone kernel with
    quota, each in a fresh child process"""
    env = dict(os.environ, KS_COMMIT_GENERAL=mode, EDGE_QUOTA="1" if quota else "0")
    plan = U.commit_plans()["general-noquota" if mode == "1" else "mono-quota"]
    assert plan["mono"] == (mode == "2") and (plan["mono"] or not plan["fq"]), plan
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    print(r.stdout[-300:])
    assert r.returncode == 0 and f"EDGE OK helpers=0 lds={plan['smem']} " in r.stdout, (plan, r.stdout[-2000:], r.stderr[-4000:])


# ---- c. the non-monotone general path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(balanced=True), dict(numa=True), dict(strategy="MostAllocated")],
                         ids=["balanced", "numa-amplified", "most-allocated"])
def test_reserve_walk_general_reevaluation(runtime, oracle_lib, kw):
    """BalancedAllocation, NodeNUMAResource with amplified CPUs (no cpuset pods) and MostAllocated are not monotone:
    the general kernel re-evaluates the touched slots"""
    U.run_reserve_walk(runtime, oracle_lib, quota=False, label=str(kw), **kw)


# ---- d. deltas across the switch ------------------------------------------------------------------------------------------

def test_node_delta_moves_a_capacity_across_the_switch(runtime, oracle_lib):
    """ks_update_nodes raises a capacity from 2^43 - 1 to 2^43 and lowers another from 2^43 to 2^43 - 1, for memory,
    LoadAware's memory and a scalar slot: kNodeBigCap has to follow.  Compared with an oracle loaded with the merged
    table: eval_pod, a queue, and the same queue again after ks_restore."""
    old = U.queue_nodes(57)
    small_nodes = [i for i in range(57) if i % 3 != 2][:6]
    up, down = small_nodes[0::2], small_nodes[1::2]
    cols = ("alloc_memory", "la_alloc_memory", ("alloc_scalar", 0))

    def col(t, c):
        return getattr(t, c[0])[c[1]] if isinstance(c, tuple) else getattr(t, c)

    for a, b, c in zip(up, down, cols):
        col(old, c)[a] = U.BIG_CAP - 1
        col(old, c)[b] = U.BIG_CAP
    new = old.copy()
    for a, b, c in zip(up, down, cols):
        col(new, c)[a] = U.BIG_CAP
        col(new, c)[b] = U.BIG_CAP - 1
    for t in (old, new):  # boundary headrooms on the switched terms
        t.nonzero_memory[up + down] = (U.BIG_CAP - 1) // 100
        t.la_term_memory[up + down] = 33 * (U.BIG_CAP - 1) // 100
    idx = np.array(sorted(up + down), np.int32)
    prof = U.queue_profile()
    cfg = prof.to_ks_config()
    ev = runtime.Evaluator(cfg, old.copy())
    orc = oracle_lib.Oracle(cfg, new.copy(), nthreads=2)
    try:
        pods = U.queue_pods(48, 2)
        ev.eval_pod(pods.rows([0]))  # the context has evaluated with the old flags
        ev.update_nodes(idx, new.rows(idx))
        for j in (0, 1, 2, 24):
            one = pods.rows([j])
            for g, w, what in zip(ev.eval_pod(one), orc.eval_pod(one), ("reasons", "scores", "total")):
                assert np.array_equal(g, w), f"after the delta, pod {j}: {what}"
        ev.checkpoint()
        want = orc.schedule(pods)
        for attempt in ("first", "after ks_restore"):
            got = ev.schedule(pods)
            for k in U.RESULT_COLS:
                assert np.array_equal(got[k], want[k]), f"queue {attempt}: {k}"
            gs, ws = ev.read_nodes().as_dict(), orc.read_nodes().as_dict()
            for k in ws:
                assert np.array_equal(gs[k], ws[k]), f"queue {attempt}: node state {k}"
            ev.restore()
        assert len(set(np.asarray(want["node"])[np.asarray(want["status"]) == 0]) & set(idx.tolist())) > 0, \
            "no pod landed on a node whose capacity crossed the switch"
    finally:
        ev.close()
        orc.close()


# ---- e. an always-int64 user: DeviceShare ------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", ["LeastAllocated", "MostAllocated"])
def test_deviceshare_at_prime_and_limit_totals(runtime, oracle_lib, strategy):
    """GPU memory totals that are prime, around 2^43 and up to 2^56 - 1 (the largest value ks_load_devices accepts),
    used amounts and requests on k c / 100 boundaries: pct_floor_i64 in ks_dev.h, through eval_pod and one queue"""
    nodes, devs, pods = U.device_workload()
    cfg = U.device_profile(strategy).to_ks_config()
    ev = runtime.Evaluator(cfg, nodes.copy(), devices=devs.copy())
    orc = oracle_lib.Oracle(cfg, nodes.copy(), devices=devs.copy(), nthreads=2)
    try:
        seen = set()
        for j in range(0, pods.n, 5):
            one = pods.rows([j])
            got, want = ev.eval_pod(one), orc.eval_pod(one)
            for g, w, what in zip(got, want, ("reasons", "scores", "total")):
                assert np.array_equal(g, w), f"pod {j}: {what}"
            seen |= set(want[1][want[0] == 0, abi.KS_SCORE_DEVICESHARE].tolist())
        assert len(seen) > 10, "the DeviceShare scores of the case do not vary"
        got, want = ev.schedule(pods), orc.schedule(pods)
        for k in U.RESULT_COLS:
            assert np.array_equal(got[k], want[k]), k
        assert (np.asarray(want["status"]) == abi.KS_S_SCHEDULED).sum() > 30
        for g, w, name in zip(ev.read_devices(), orc.read_devices(), ("core", "memory", "ratio", "rdma")):
            assert np.array_equal(g, w), f"device used {name}"
        bad = devs.copy()
        bad.total_memory[0, 0] = U.LIMIT
        with pytest.raises(runtime.KsError) as ei:
            ev.load_devices(bad)
        assert ei.value.rc == abi.KS_EINVAL
    finally:
        ev.close()
        orc.close()


def eval_and_queue(ev, orc, pods, col, label, step=3):
    """eval_pod of every step-th pod and then the queue, device against oracle; returns the values seen in score
    column col on feasible nodes and the oracle's results"""
    seen = set()
    for j in range(0, pods.n, step):
        one = pods.rows([j])
        got, want = ev.eval_pod(one), orc.eval_pod(one)
        for g, w, what in zip(got, want, ("reasons", "scores", "total")):
            assert np.array_equal(g, w), f"{label} pod {j}: {what}"
        seen |= set(want[1][want[0] == 0, col].tolist())
    got, want = ev.schedule(pods), orc.schedule(pods)
    for k in U.RESULT_COLS:
        assert np.array_equal(got[k], want[k]), f"{label}: {k}"
    gs, ws = ev.read_nodes().as_dict(), orc.read_nodes().as_dict()
    for k in ws:
        assert np.array_equal(gs[k], ws[k]), f"{label}: node state {k}"
    return seen, want


def test_reservation_at_boundary_allocatables(runtime, oracle_lib):
    """scoreReservation (ks_rsv.h rsv_score): memory allocatable 2^55 + 7, 2^43 - 1, 2^43, 2^43 + 1 and primes,
    (request + allocated) / allocatable on k / 100 boundaries; eval_pod and one queue of 64 pods"""
    nodes, rs, pods = U.reservation_workload()
    cfg = U.reservation_profile().to_ks_config()
    ev = runtime.Evaluator(cfg, nodes.copy(), reservations=rs.copy())
    orc = oracle_lib.Oracle(cfg, nodes.copy(), reservations=rs.copy(), nthreads=2)
    try:
        seen, want = eval_and_queue(ev, orc, pods, abi.KS_SCORE_RESERVATION, "reservation")
        assert len(seen) > 5, "the Reservation scores of the case do not vary"
        assert (np.asarray(want["reservation"]) >= 0).sum() > 30, "few pods were placed into a reservation"
        for g, w in zip(ev.read_reservations(), orc.read_reservations()):
            assert np.array_equal(g, w), "reservation allocated / assigned"
    finally:
        ev.close()
        orc.close()


@pytest.mark.parametrize("strategy", ["LeastAllocated", "MostAllocated"])
def test_numa_policy_nodes_at_the_loader_limit(runtime, oracle_lib, strategy):
    """numa_res_score (ks_numa.h): per-NUMA cpu and memory of 2^50 (the largest ks_load_numa_nodes accepts), just
    under it and a prime, used amounts and requests on k c / 100 boundaries; eval_pod and one queue of 64 pods"""
    nodes, nn, pods = U.numa_policy_workload()
    cfg = U.numa_policy_profile(strategy).to_ks_config()
    ev = runtime.Evaluator(cfg, nodes.copy(), numa_nodes=nn.copy())
    orc = oracle_lib.Oracle(cfg, nodes.copy(), numa_nodes=nn.copy(), nthreads=2)
    try:
        seen, want = eval_and_queue(ev, orc, pods, abi.KS_SCORE_NUMA, f"numa-policy-{strategy}")
        assert len(seen) > 5, "the NodeNUMAResource scores of the case do not vary"
        assert (np.asarray(want["status"]) == abi.KS_S_SCHEDULED).sum() > 30
        for g, w in zip(ev.read_numa_nodes(), orc.read_numa_nodes()):
            assert np.array_equal(g, w), "NUMA allocatedResources"
        bad = nn.copy()
        bad.alloc_memory[0, 0] = U.NUMA_LIMIT + 1
        with pytest.raises(runtime.KsError) as ei:
            ev.load_numa_nodes(bad)
        assert ei.value.rc == abi.KS_EINVAL
    finally:
        ev.close()
        orc.close()


# ---- f. pod values outside the validated range --------------------------------------------------------------------------

POD_COLUMNS = ("req_milli_cpu", "req_memory", "req_ephemeral", "nonzero_milli_cpu", "nonzero_memory", "la_req_cpu",
               "la_lim_cpu", "la_req_memory", "la_lim_memory", "la_dflt_cpu", "la_dflt_memory")


def test_pod_quantities_outside_the_range_are_refused(runtime, oracle_lib):
    """ks_schedule / ks_stage_pods / ks_eval_pod refuse a pod quantity outside [0, 2^56) with KS_EINVAL, as node columns
    are refused: a negative request would reach pct_floor_i64 with num > cap, and 100 * num can leave int64.  The
    LoadAware default estimates (la_dflt_*) are score-term requests too.  The largest accepted value, 2^56 - 1, scores
    as the oracle does."""
    nodes = U.queue_nodes(57)
    cfg = U.queue_profile().to_ks_config()
    ev = runtime.Evaluator(cfg, nodes.copy())
    orc = oracle_lib.Oracle(cfg, nodes.copy())
    try:
        for name in POD_COLUMNS + (("req_scalar", 0),):
            for bad in (-1, -(1 << 62), U.LIMIT, (1 << 63) - 1):
                pods = U.queue_pods(3)
                a = getattr(pods, name[0])[name[1]] if isinstance(name, tuple) else getattr(pods, name)
                a[1] = bad
                for call in (lambda: ev.schedule(pods), lambda: ev.stage(pods), lambda: ev.eval_pod(pods.rows([1]))):
                    with pytest.raises(runtime.KsError) as ei:
                        call()
                    assert ei.value.rc == abi.KS_EINVAL, (name, bad, ei.value)
            pods = U.queue_pods(3)
            a = getattr(pods, name[0])[name[1]] if isinstance(name, tuple) else getattr(pods, name)
            a[1] = U.LIMIT - 1
            if name == ("req_scalar", 0):
                pods.flags[1] |= abi.KS_POD_SCALAR_KEYS
            one = pods.rows([1])
            for g, w, what in zip(ev.eval_pod(one), orc.eval_pod(one), ("reasons", "scores", "total")):
                assert np.array_equal(g, w), f"{name} = 2^56 - 1: {what}"
        # the context still schedules after the refusals
        pods = U.queue_pods(20)
        got, want = ev.schedule(pods), orc.schedule(pods)
        for k in U.RESULT_COLS:
            assert np.array_equal(got[k], want[k]), k
    finally:
        ev.close()
        orc.close()
