"""DeviceShare's reservation path on the device against the reference's own test tables
(tests/golden/deviceshare_reservation_plugin.json: TestScoreReservation, Test_Plugin_FilterReservation, the reservation /
preemptible cases of Test_Plugin_Filter / Test_Plugin_Reserve / Test_Plugin_Unreserve and
Test_failedPreemptGPUFromReservation), through ks_eval_pod, ks_eval_pod_summary, ks_assume / ks_unreserve and
ks_schedule.  Every expected value comes from the fixture; device == oracle is asserted next to it, so that a failure
says which side is wrong.  Hand-built edge clusters (rsv_plugin_util.edge_scenarios, checked on the oracle in
test_deviceshare_reservation_golden.py) follow.  All values are integers and compared exactly."""
import numpy as np
import pytest

import rsv_plugin_util as U
from helpers import assert_same_results, assert_same_state
from koordinator_amd import abi

pytestmark = pytest.mark.gpu
P = U.G
DS = abi.KS_SCORE_DEVICESHARE


@pytest.fixture(scope="module")
def runtime():
    from koordinator_amd import runtime as rt

    rt.lib()
    return rt


def pair(runtime, oracle_lib, specs, strategy="LeastAllocated"):
    nodes, rs, dev, first = U.tables(specs)
    cfg = U.config(strategy)
    r = rs if rs.r else None
    return (runtime.Evaluator(cfg, nodes.copy(), reservations=r, devices=dev.copy()),
            oracle_lib.Oracle(cfg, nodes.copy(), reservations=r, devices=dev.copy()), rs, first)


def same_eval(ev, orc, pod):
    g, o = ev.eval_pod(pod), orc.eval_pod(pod)
    for a, b, what in zip(g, o, ("reasons", "scores", "totals")):
        assert np.array_equal(a, b), f"device != oracle: {what}: {a.tolist()} vs {b.tolist()}"
    return g


def same_state(ev, orc, label):
    for a, b in zip(U.snapshot(ev), U.snapshot(orc)):
        assert a == b, f"{label}: device / reservation state differs from the oracle"
    assert_same_state(ev.read_nodes(), orc.read_nodes(), label)


def assume_both(ev, orc, pod, node, label):
    """ks_assume and ko_assume on `node`; returns the device's record and the undo"""
    before = U.snapshot(ev)
    rg, cg, ng = ev.assume(pod, node)
    ro, co, no = orc.assume(pod, node)
    for k in ("node", "status", "reservation", "gpu_minors", "rdma_minors"):
        assert rg[k][0] == ro[k][0], f"{label}: device {k} {rg[k][0]} != oracle {ro[k][0]}"
    same_state(ev, orc, label + " after assume")

    def undo():
        ev.unreserve(pod, rg, cg, ng)
        orc.unreserve(pod, ro, co, no)
        assert U.snapshot(ev) == before, f"{label}: unreserve does not restore the bytes before the assume"
        same_state(ev, orc, label + " after unreserve")

    return rg, undo


def schedule_both(runtime, oracle_lib, specs, strategy, pod_spec, copies, label):
    """the batched path: a queue of `copies` pods through ks_schedule (the commit kernels' held variants)"""
    ev, orc, rs, _ = pair(runtime, oracle_lib, specs, strategy)
    try:
        pods = U.pod_of(pod_spec, copies)
        got, want = ev.schedule(pods), orc.schedule(pods)
        assert_same_results(got, want, label)
        for k in ("reservation", "gpu_minors", "rdma_minors"):
            assert np.array_equal(got[k], want[k]), f"{label}: {k}: {got[k].tolist()} vs {want[k].tolist()}"
        same_state(ev, orc, label)
        rd = ev.read_reservation_devices()
    finally:
        ev.close()
        orc.close()
    return got, rd, rs


@pytest.mark.parametrize("strategy,pod_spec,cases", U.score_groups(), ids=lambda v: v if isinstance(v, str) else None)
def test_score_reservation_group(runtime, oracle_lib, strategy, pod_spec, cases):
    """One cluster per (strategy, pod request), each TestScoreReservation case one node with its one matched, passing
    reservation: the reservation is nominated, so DeviceShare's Score is the ScoreReservation value (scoring.go:72-76)
    and the DeviceShare column is 100 * want_i / max(want) from the fixture.  The GPU + RDMA case (raw 120) is a group of
    one, which always normalizes to 100: no TestScore entry of tests/golden/deviceshare.json has its request (gpu 50 /
    50 with rdma 20), so there is no pinned second node to make the ratio informative; that case rests on the assume
    checks here (minors, reservation, allocation per minor) and on the oracle hook's raw 120."""
    specs = [U.case_node(c, U.SCORE["gpus"], U.SCORE["rdma"]) for c in cases]
    want = U.normalized([c["want_score"] for c in cases])
    ev, orc, rs, first = pair(runtime, oracle_lib, specs, strategy)
    try:
        pod = U.pod_of(pod_spec)
        reasons, scores, totals = ev.eval_pod(pod)
        assert not reasons.any(), reasons.tolist()
        assert scores[:, DS].tolist() == want, f"device DeviceShare column {scores[:, DS].tolist()}, fixture {want}"
        same_eval(ev, orc, pod)
        # the same cluster reduced on the device
        s = ev.eval_pod_summary(pod, top_n=len(cases))
        order = sorted(range(len(cases)), key=lambda i: (-int(totals[i]), i))
        assert s["feasible"] == len(cases) and s["best_node"] == order[0] and s["best_total"] == totals[order[0]]
        assert s["top_nodes"].tolist() == order and s["top_totals"].tolist() == [int(totals[i]) for i in order]
        assert s["top_scores"][:, DS].tolist() == [want[i] for i in order]
        # Reserve into the nominated reservation, then Unreserve, per case
        for i, c in enumerate(cases):
            rec, undo = assume_both(ev, orc, pod, i, c["ref"])
            assert rec["status"][0] == abi.KS_S_SCHEDULED and rec["reservation"][0] == first[i], c["ref"]
            assert U.minor_list(rec["gpu_minors"][0]) == [0], c["ref"]
            assert U.minor_list(rec["rdma_minors"][0]) == ([0] if pod_spec["rdma"] else []), c["ref"]
            # the pod's allocation: 50 / 8Gi / 50 on the reservation's minor; the RDMA share is not the reservation's
            alloc = U.words({"0": [pod_spec["core"], 16 * pod_spec["ratio"] // 100, pod_spec["ratio"]]})
            assert np.array_equal(ev.read_reservation_devices()[first[i]], alloc), c["ref"]
            used = ev.read_devices()
            u0 = U.words(c["used_at_call"])
            assert used[0][0, i] == u0[abi.dev_word("gpu", 0, 0)] + pod_spec["core"]
            assert used[2][0, i] == u0[abi.dev_word("gpu", 0, 2)] + pod_spec["ratio"]
            assert used[3][0, i] == pod_spec["rdma"]
            assert ev.read_reservations()[1][first[i]] == 1
            undo()
    finally:
        ev.close()
        orc.close()
    got, rd, _ = schedule_both(runtime, oracle_lib, specs, strategy, pod_spec, min(4, max(2, len(cases))), "queue")
    # (later copies may find every reservation and node used up; the first pod always has its place and its minor)
    assert got["status"][0] == abi.KS_S_SCHEDULED and got["gpu_minors"][0] == 1 and got["reservation"][0] >= 0


def test_filter_reservation_pair(runtime, oracle_lib):
    """Test_Plugin_FilterReservation on a node whose GPUs are minors 1 and 2: nominated before the assigned pod, not
    after it"""
    f = P["filter_reservation"]
    pod = U.pod_of(f["pod"])

    def node(phase):
        ph = f[phase]
        return {"gpus": f["gpus"], "used": ph["used_at_call"],
                "rows": [U.row(f["policy"], U.words(f["reserved"]), U.words(ph["assigned_allocated"]), ph["assigned"])]}

    ev, orc, _, _ = pair(runtime, oracle_lib, [node("before")])
    try:
        reasons, _, _ = same_eval(ev, orc, pod)
        assert f["before"]["want"] == "pass" and reasons[0] == 0
        rec, undo = assume_both(ev, orc, pod, 0, "before")
        assert rec["reservation"][0] == 0 and U.minor_list(rec["gpu_minors"][0]) == [1]
        assert np.array_equal(ev.read_reservation_devices()[0], U.words(f["reserved"]))
        undo()
    finally:
        ev.close()
        orc.close()
    ev, orc, _, _ = pair(runtime, oracle_lib, [node("after")])
    try:
        reasons, _, _ = same_eval(ev, orc, pod)
        # no reservation meets the device requirements, and the plain node is full (plugin.go:316-321)
        assert reasons[0] == abi.KS_R_DEV_INSUFFICIENT
        got, want = ev.schedule(pod), orc.schedule(pod)
        assert_same_results(got, want, "after")
        assert got["reservation"][0] == -1 and got["status"][0] != abi.KS_S_SCHEDULED and got["gpu_minors"][0] == 0
    finally:
        ev.close()
        orc.close()


@pytest.mark.parametrize("case", P["filter"]["cases"] + P["reserve"]["cases"], ids=lambda c: c["ref"])
def test_filter_and_reserve_cases(runtime, oracle_lib, case):
    """Filter's verdict, Reserve's allocation per minor and the reservation it goes into, Unreserve back"""
    pod = U.pod_of(case["pod"])
    ev, orc, rs, _ = pair(runtime, oracle_lib, [U.case_node(case)])
    try:
        reasons, _, _ = same_eval(ev, orc, pod)
        assert reasons[0] == 0, case["name"]
        used0 = [a.copy() for a in ev.read_devices()]
        rd0 = ev.read_reservation_devices().copy()
        rec, undo = assume_both(ev, orc, pod, 0, case["ref"])
        assert rec["status"][0] == abi.KS_S_SCHEDULED
        if "want_allocation" in case:
            want = U.words(case["want_allocation"])
            assert U.minor_list(rec["gpu_minors"][0]) == [int(k) for k in case["want_allocation"]]
            used1 = ev.read_devices()
            got = np.zeros(abi.KS_DEV_WORDS, np.int64)
            for q in range(3):
                for k in range(abi.KS_MAX_GPUS):
                    got[abi.dev_word("gpu", k, q)] = used1[q][k, 0] - used0[q][k, 0]
            assert np.array_equal(got, want)
            grew = ev.read_reservation_devices() - rd0
            if case["want_nominated"]:
                assert rec["reservation"][0] == 0 and np.array_equal(grew[0], want)
                assert ev.read_reservations()[1][0] == 1
            else:
                assert rec["reservation"][0] == -1 and not grew.any()
        undo()
    finally:
        ev.close()
        orc.close()
    schedule_both(runtime, oracle_lib, [U.case_node(case)], "LeastAllocated", case["pod"], 2, case["ref"])


def test_unreserve_normal_case(runtime, oracle_lib):
    u = P["unreserve"]
    pod = U.pod_of(u["pod"])
    ev, orc, _, _ = pair(runtime, oracle_lib, [{"gpus": u["gpus"], "rdma": u["rdma"], "used": {}, "rows": []}])
    try:
        rec, undo = assume_both(ev, orc, pod, 0, "unreserve")
        assert U.minor_list(rec["gpu_minors"][0]) == [int(k) for k in u["allocation"]["gpu"]]
        assert U.minor_list(rec["rdma_minors"][0]) == [int(k) for k in u["allocation"]["rdma"]]

        def used_words():
            d = ev.read_devices()
            w = np.zeros(abi.KS_DEV_WORDS, np.int64)
            for k in range(abi.KS_MAX_GPUS):
                for q in range(3):
                    w[abi.dev_word("gpu", k, q)] = d[q][k, 0]
            for k in range(abi.KS_MAX_RDMA):
                w[abi.dev_word("rdma", k)] = d[3][k, 0]
            return w

        assert np.array_equal(used_words(), U.words(u["used_before"]["gpu"], u["used_before"]["rdma"]))
        undo()
        assert np.array_equal(used_words(), U.words(u["used_after"]["gpu"], u["used_after"]["rdma"]))
    finally:
        ev.close()
        orc.close()


def test_failed_preempt_from_reservation(runtime, oracle_lib):
    """used 200 of 100 with 100 given back: used' = 100, free = max(0, 100 - 100) = 0 -> Insufficient gpu devices"""
    f = P["failed_preempt"]
    pod = U.pod_of(f["pod"])
    ev, orc, _, _ = pair(runtime, oracle_lib, [U.case_node(f)])
    try:
        reasons, _, _ = same_eval(ev, orc, pod)
        assert f["want"] == "Insufficient gpu devices" and reasons[0] == abi.KS_R_DEV_INSUFFICIENT
        s = ev.eval_pod_summary(pod)
        assert s["feasible"] == 0 and s["best_node"] == -1
    finally:
        ev.close()
        orc.close()


@pytest.mark.parametrize("sc", U.edge_scenarios(), ids=lambda s: s["name"][:50])
def test_edge_clusters(runtime, oracle_lib, sc):
    """Hand-built edge clusters: the nomination, the Filter verdict, Reserve's minors and the growth of the nominated
    reservation's device allocation are the hand-derived ones of the scenario, on the device as on the oracle; then the
    same pod twice through ks_schedule.  The first scenario is the one where Filter passes on another reservation than
    the nominated one (the commit kernels take the minors of the nominated view): the placed pod has its minors and
    the nominated reservation's allocation grows by the request.  A state where Reserve on the nominated view fails
    cannot be built through the tables: the nominated reservation passed FilterReservation's allocation on the same
    view, and Reserve's scorer only reorders minors that fit."""
    got_d = U.run_scenario(lambda cfg, n, rs, dev: runtime.Evaluator(cfg, n, reservations=rs, devices=dev), sc)
    got_o = U.run_scenario(lambda cfg, n, rs, dev: oracle_lib.Oracle(cfg, n, reservations=rs, devices=dev), sc)
    for k in ("reasons", "scores", "totals"):
        assert np.array_equal(got_d[k], got_o[k]), f"{sc['name']}: device != oracle: {k}"
    assert got_d["state"] == got_o["state"], f"{sc['name']}: state after assume differs from the oracle"
    got, rd, rs = schedule_both(runtime, oracle_lib, sc["nodes"], sc["strategy"], sc["pod"], 2, sc["name"])
    w = sc["want"]
    assert got["status"][0] == abi.KS_S_SCHEDULED and U.minor_list(got["gpu_minors"][0]) == w["gpu"]
    assert got["reservation"][0] == w["nominated"]
    for i in range(2):
        assert got["status"][i] != abi.KS_S_SCHEDULED or got["gpu_minors"][i] != 0, "scheduled without minors"
    if w["nominated"] >= 0:
        assert (rd[w["nominated"]] - rs.dev_allocated[w["nominated"]]).any()
