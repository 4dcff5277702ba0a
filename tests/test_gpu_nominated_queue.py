"""The batched queue with a nominated table loaded (ks_schedule_nominated, ks_stage_pods_nominated +
ks_schedule_staged + ks_fetch_results; the NOM variants of the sweep and the general commit, nom_retire_kernel,
koordinator_amd/csrc/ks_nominated.h) against the reference composed from the unchanged CPU oracle
(tests/nominated_queue_ref.py, pinned and checked for non-vacuity by tests/test_nominated_queue_ref.py).  Every
comparison is exact.

200 nodes, 192 pods = three 64-pod windows; ~90 rows on 10 nodes (70 on one); 8 owner pods: the queue's first pod,
both sides of a window boundary, two adjacent ones, one whose nominated node is full, one its quota rejects."""
import numpy as np
import pytest

import nominated_queue_ref as qref
import nominated_ref as ref
from koordinator_amd import abi

pytestmark = pytest.mark.gpu

IDS = ["c2", "c2-taint-affinity"]
_cases = {}


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()  # the in-tree HIP library; no fallback
    return rt


def case(oracle_lib, static):
    """the workload and its reference, computed once per module and left unchanged"""
    if static not in _cases:
        w, nom, prio, nn, sid = qref.workload(static)
        want = qref.schedule(oracle_lib, w.cfg, w.nodes, w.quotas, nom, w.pods, prio, nn, sid)
        _cases[static] = (w, nom, prio, nn, sid, want)
    return _cases[static]


def evaluator(runtime, w, nom=None):
    ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
    if nom is not None:
        ev.load_nominated(nom)
    return ev


def check_results(got, want, label):
    for k in ("status", "node", "score"):
        bad = np.flatnonzero(got[k] != want[k])
        assert not len(bad), f"{label}: {k} differs at pods {bad[:10]}: {got[k][bad[:10]]} != {want[k][bad[:10]]}"


def check_state(ev, want, label):
    gs = ev.read_nodes().as_dict()
    for k, v in want["nodes"].items():
        assert np.array_equal(gs[k], v), f"{label}: node state {k}"
    assert np.array_equal(ev.read_quota_used(), want["quota_used"]), f"{label}: quota usage"


def check_surviving_table(oracle_lib, ev, w, want, label):
    """a probe pod's evaluation after the call equals the reference's on the surviving rows and the final state"""
    nodes = w.nodes.copy()
    for k, v in want["nodes"].items():
        if k not in ("host_ports", "topo_count"):
            getattr(nodes, k)[...] = v
    q = w.quotas.copy()
    q.used[:] = want["quota_used"].T
    probe = w.pods.rows([1])
    for prio in (400, 1000, 1501):
        e = ref.evaluate(oracle_lib, w.cfg, nodes, {"quotas": q}, want["live"], probe, priority=prio)
        r, s, t = ev.eval_pod_nominated(probe, priority=prio)
        assert np.array_equal(r, e["reasons"]), f"{label}: probe priority {prio}: reasons at {np.flatnonzero(r != e['reasons'])}"
        assert np.array_equal(s, e["scores"]) and np.array_equal(t, e["total"]), f"{label}: probe priority {prio}: scores"


@pytest.mark.parametrize("static", [False, True], ids=IDS)
def test_queue_against_the_composed_reference(runtime, oracle_lib, static):
    w, nom, prio, nn, sid, want = case(oracle_lib, static)
    ev = evaluator(runtime, w, nom)
    try:
        ev.set_pipeline(2)  # asked for, not used while a table is loaded
        got = ev.schedule_nominated(w.pods, prio, nn, sid)
        check_results(got, want, "schedule_nominated")
        check_state(ev, want, "schedule_nominated")
        check_surviving_table(oracle_lib, ev, w, want, "schedule_nominated")
        st = ev.stats()
        owners_ok = [i for i in qref.OWNER_POS if want["status"][i] == abi.KS_S_SCHEDULED]
        assert st["pipelined"] == 0
        assert st["diag"][4] == len(qref.OWNER_POS), "owner passes"
        assert st["diag"][5] == len(owners_ok) == nom.m - want["live"].m, "retired rows"
        assert st["cut_passes"] >= len(qref.OWNER_POS) - 1
        # a retired id has no row: deleting it changes nothing
        ev.delete_nominated([int(sid[owners_ok[0]])])
        check_surviving_table(oracle_lib, ev, w, want, "after the no-op delete")
    finally:
        ev.close()


@pytest.mark.parametrize("static", [False, True], ids=IDS)
def test_staged_trio_gives_the_same_results(runtime, oracle_lib, static):
    w, nom, prio, nn, sid, want = case(oracle_lib, static)
    ev = evaluator(runtime, w, nom)
    try:
        ev.stage_nominated(w.pods, prio, nn, sid)
        ev.schedule_staged()
        check_results(ev.fetch(), want, "staged")
        check_state(ev, want, "staged")
    finally:
        ev.close()


def test_checkpoint_schedule_restore_schedule(runtime, oracle_lib):
    w, nom, prio, nn, sid, want = case(oracle_lib, False)
    ev = evaluator(runtime, w, nom)
    try:
        ev.checkpoint()
        for rnd in range(2):
            check_results(ev.schedule_nominated(w.pods, prio, nn, sid), want, f"round {rnd}")
            check_state(ev, want, f"round {rnd}")
            ev.restore()
        # the table came back with the state: the first probe of the untouched context
        probe = w.pods.rows([1])
        e = ref.evaluate(oracle_lib, w.cfg, w.nodes, w.tables(), nom, probe, priority=400)
        r, s, t = ev.eval_pod_nominated(probe, priority=400)
        assert np.array_equal(r, e["reasons"]) and np.array_equal(t, e["total"])
    finally:
        ev.close()


@pytest.mark.parametrize("static", [False, True], ids=IDS)
def test_empty_table_equals_schedule(runtime, oracle_lib, static):
    w, nom, prio, nn, sid, _ = case(oracle_lib, static)
    plain, none, emptied = (evaluator(runtime, w) for _ in range(3))
    try:
        emptied.load_nominated(nom)
        emptied.load_nominated(None)
        want = plain.schedule(w.pods)
        for ev, label in ((none, "no table"), (emptied, "emptied table")):
            got = ev.schedule_nominated(w.pods, prio, nn, sid)
            for k in ("status", "node", "score"):
                assert np.array_equal(got[k], want[k]), f"{label}: {k}"
    finally:
        for ev in (plain, none, emptied):
            ev.close()


def test_refusals_and_validation(runtime, oracle_lib):
    w, nom, prio, nn, sid, _ = case(oracle_lib, False)
    ev = evaluator(runtime, w, nom)
    try:
        for bad in (w.nodes.n, -2):
            x = nn.copy()
            x[5] = bad
            with pytest.raises(runtime.KsError) as e:
                ev.schedule_nominated(w.pods, prio, x, sid)
            assert e.value.rc == abi.KS_EINVAL
        x = sid.copy()
        x[7] = x[qref.OWNER_POS[1]]
        with pytest.raises(runtime.KsError) as e:
            ev.schedule_nominated(w.pods, prio, nn, x)
        assert e.value.rc == abi.KS_EINVAL and "twice" in str(e.value)
        x = sid.copy()
        x[7] = -2
        with pytest.raises(runtime.KsError) as e:
            ev.stage_nominated(w.pods, prio, nn, x)
        assert e.value.rc == abi.KS_EINVAL
        # the old staging entry point still refuses, and what it did not stage is not scheduled
        with pytest.raises(runtime.KsError) as e:
            ev.stage(w.pods)
        assert e.value.rc == abi.KS_EUNSUPPORTED
    finally:
        ev.close()
    # node sharding with a table
    ranks = [evaluator(runtime, w), evaluator(runtime, w)]
    try:
        runtime.shard_loopback(ranks)
        ranks[0].load_nominated(nom)
        with pytest.raises(runtime.KsError) as e:
            ranks[0].schedule_nominated(w.pods, prio, nn, sid)
        assert e.value.rc == abi.KS_EUNSUPPORTED and "shard" in str(e.value)
    finally:
        for r in ranks:
            r.close()


def test_rescan_applies_the_table(runtime, oracle_lib):
    """one chunk whose best and runner-up are touched by the pass's first two pods: the later pods are resolved by
    re-scanning the chunk's untouched nodes, among them a nominated node that is closed to them and would win on its
    plain row (premises: tests/test_nominated_queue_ref.py)"""
    w, nom, prio = qref.rescan_workload(oracle_lib)
    want = qref.schedule(oracle_lib, w.cfg, w.nodes, w.quotas, nom, w.pods, prio)
    ev = evaluator(runtime, w, nom)
    try:
        got = ev.schedule_nominated(w.pods, prio)
        st = ev.stats()
        print("rescans", st["rescans"], "passes", st["passes"], "cut", st["cut_passes"], "nodes", got["node"])
        check_results(got, want, "rescan")
        check_state(ev, want, "rescan")
        assert st["rescans"] > 0
        assert not (got["node"] == qref.RESCAN_NOM).any()
    finally:
        ev.close()
