"""DeviceShare with reservations that hold devices (deviceshare/reservation.go) on the C oracle, pinned by the
reference's own tests (tests/golden/deviceshare_reservation.json, transcribed from deviceshare/reservation_test.go):
RestoreReservation's merged restore state (Test_Plugin_ReservationRestore) and tryAllocateFromReservation over the
Default / Aligned / Restricted policies (Test_tryAllocateFromReservation), through test hooks of the oracle."""
import ctypes as C
import json
import pathlib

import numpy as np
import pytest

from koordinator_amd import abi, synth
from koordinator_amd.cluster import DeviceTable, NodeTable, PodTable, ReservationTable
from koordinator_amd.config import DeviceShareArgs
from oracle.oracle import Oracle

G = json.loads((pathlib.Path(__file__).parent / "golden" / "deviceshare_reservation.json").read_text())
GIB = G["gib"]
POLICY = {"Default": abi.KS_RSV_POLICY_DEFAULT, "Aligned": abi.KS_RSV_POLICY_ALIGNED,
          "Restricted": abi.KS_RSV_POLICY_RESTRICTED}


def words(minors: dict) -> np.ndarray:
    w = np.zeros(abi.KS_DEV_WORDS, np.int64)
    for k, (core, mem, ratio) in minors.items():
        k = int(k)
        w[abi.dev_word("gpu", k, 0)] = core
        w[abi.dev_word("gpu", k, 1)] = mem * GIB
        w[abi.dev_word("gpu", k, 2)] = ratio
    return w


def cluster(gpus: dict, used: dict, rows: list):
    nodes = NodeTable(1)
    nodes.alloc_milli_cpu[:] = 64000
    nodes.alloc_memory[:] = 256 * GIB
    nodes.allowed_pods[:] = 110
    dev = DeviceTable(1)
    dev.flags[:] = abi.KS_DEV_PRESENT
    for k, (core, mem, ratio) in gpus.items():
        dev.total_core[int(k), 0], dev.total_memory[int(k), 0], dev.total_ratio[int(k), 0] = core, mem * GIB, ratio
    for k, (core, mem, ratio) in used.items():
        dev.used_core[int(k), 0], dev.used_memory[int(k), 0], dev.used_ratio[int(k), 0] = core, mem * GIB, ratio
    rs = ReservationTable(len(rows)).hold_devices()
    for i, (pol, al, ald, assigned) in enumerate(rows):
        rs.owner_classes[i] = 1
        rs.policy[i] = pol
        rs.key_mask[i] = 0b11
        rs.allocatable[0, i] = 1000
        rs.assigned[i] = assigned
        rs.dev_allocatable[i] = al
        rs.dev_allocated[i] = ald
    prof = synth.koord_profile(with_reservation=True)
    prof.deviceshare = DeviceShareArgs()
    return Oracle(prof.to_ks_config(), nodes, reservations=rs, devices=dev)


def gpu_pod(core: int, mem_or_ratio: int, by_memory: bool) -> PodTable:
    p = PodTable(1)
    p.req_milli_cpu[:] = 100
    p.nonzero_milli_cpu[:] = 100
    p.nonzero_memory[:] = 200 << 20
    p.rsv_class[:] = 0
    p.gpu_core[:] = core
    if by_memory:
        p.gpu_memory[:] = mem_or_ratio * GIB
        p.flags[:] = abi.KS_POD_GPU_CORE | abi.KS_POD_GPU_MEMORY
    else:
        p.gpu_memory_ratio[:] = mem_or_ratio
        p.flags[:] = abi.KS_POD_GPU_CORE
    return p


def test_reservation_restore_state():
    c = G["restore"]
    r = c["reservation"]
    orc = cluster(c["gpus"], c["used"], [(abi.KS_RSV_POLICY_DEFAULT, words(r["allocatable"]), words(r["allocated"]),
                                          r["assigned"])])
    pod = gpu_pod(c["pod"]["core"], c["pod"]["ratio"], False)
    pc = pod.ks()
    uu, mm, am = (np.zeros(abi.KS_DEV_WORDS, np.int64) for _ in range(3))
    orc.L.ko_test_device_restore.argtypes = [C.c_void_p, C.POINTER(abi.KsPodCols), C.c_int64, abi.P64, abi.P64, abi.P64]
    nm = orc.L.ko_test_device_restore(orc.h, C.byref(pc), 0, *(a.ctypes.data_as(abi.P64) for a in (uu, mm, am)))
    w = c["want"]
    assert nm == w["matched"]
    assert np.array_equal(uu, words(w["merged_unmatched_used"]))
    assert np.array_equal(am, words(w["merged_matched_allocatable"]))
    assert np.array_equal(mm, words(w["merged_matched_allocated"]))
    orc.close()


@pytest.mark.parametrize("case", G["try_allocate"]["cases"], ids=lambda c: c["name"][:60])
def test_try_allocate_from_reservation(case):
    rows = [(POLICY[m["policy"]], words(m["allocatable"]), words(m["allocatable"]) - words(m["remained"]), 1)
            for m in case["matched"]]
    orc = cluster(G["try_allocate"]["gpus"], case["used"], rows or [(0, np.zeros(abi.KS_DEV_WORDS, np.int64),
                                                                     np.zeros(abi.KS_DEV_WORDS, np.int64), 0)])
    pod = gpu_pod(case["pod"][0], case["pod"][1], True)
    pc = pod.ks()
    idx = np.arange(len(case["matched"]), dtype=np.int32)
    uu = np.zeros(abi.KS_DEV_WORDS, np.int64)
    mm = words(case["mm"])
    out = np.zeros(2, np.uint32)
    L = orc.L
    L.ko_test_try_reservation.argtypes = [C.c_void_p, C.POINTER(abi.KsPodCols), C.c_int64, abi.P32, C.c_int32, abi.P64,
                                          abi.P64, C.c_int32, abi.PU32]
    rc = L.ko_test_try_reservation(orc.h, C.byref(pc), 0, idx.ctypes.data_as(abi.P32), len(idx),
                                   uu.ctypes.data_as(abi.P64), mm.ctypes.data_as(abi.P64), int(case["required"]),
                                   out.ctypes.data_as(abi.PU32))
    want = case["want"]
    if want is None:
        assert rc == 0
    elif want == "unschedulable":
        assert rc == -1
    else:
        assert rc == 1 and out[0] == sum(1 << k for k in want) and out[1] == 0
    orc.close()


# ---- the plugin-level tables (tests/golden/deviceshare_reservation_plugin.json): TestScoreReservation,
# Test_Plugin_FilterReservation, the reservation / preemptible cases of Test_Plugin_Filter, Test_Plugin_Reserve and
# Test_Plugin_Unreserve, Test_failedPreemptGPUFromReservation.  Every value is an integer, every comparison exact.

import rsv_plugin_util as U  # noqa: E402

P = U.G


def oracle_of(node_specs, strategy="LeastAllocated"):
    nodes, rs, dev, first = U.tables(node_specs)
    return Oracle(U.config(strategy), nodes, reservations=rs if rs.r else None, devices=dev), first


def candidate(orc, pod, node, rows, pre=None, node_reason=False):
    """ko_test_rsv_candidate: (pass [m], raw [m], normalized [m], Filter reason on the node or None)"""
    L = orc.L
    L.ko_test_rsv_candidate.argtypes = [C.c_void_p, C.POINTER(abi.KsPodCols), C.c_int64, abi.P32, C.c_int32, abi.P64,
                                        abi.P32, abi.P64, abi.P64, abi.PU32]
    rows = np.asarray(rows, np.int32)
    m = len(rows)
    ok, raw, norm = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
    nr = np.zeros(1, np.uint32)
    pc = pod.ks()
    prev = None if pre is None else np.ascontiguousarray(pre, np.int64)
    rc = L.ko_test_rsv_candidate(orc.h, C.byref(pc), node, rows.ctypes.data_as(abi.P32), m,
                                 prev.ctypes.data_as(abi.P64) if prev is not None else None, ok.ctypes.data_as(abi.P32),
                                 raw.ctypes.data_as(abi.P64), norm.ctypes.data_as(abi.P64),
                                 nr.ctypes.data_as(abi.PU32) if node_reason else None)
    assert rc == 0
    return ok[:m], raw[:m], norm[:m], int(nr[0]) if node_reason else None


def test_fixture_cases_carry_refs():
    cases = (U.SCORE["cases"] + P["filter"]["cases"] + P["reserve"]["cases"] +
             [P["filter_reservation"], P["filter_reservation"]["before"], P["filter_reservation"]["after"], P["unreserve"],
              P["failed_preempt"]])
    assert len(U.SCORE["cases"]) == 9
    for c in cases:
        assert ":" in c["ref"], c
    assert [c["want_score"] for c in U.SCORE["cases"]] == [25, 75, 25, 75, 0, 100, 50, 50, 120]


# every case through the unmatched-reservation mapping; the ones with a preemptible vector also as the reference states
# them; the derived clamp case (a preemptible amount above the usage has no table form) only so
HOOK_CASES = ([(c, False) for c in U.SCORE["cases"]] + [(c, True) for c in U.SCORE["cases"] if c["preemptible"]] +
              [(P["derived"]["clamp_case"], True)])


@pytest.mark.parametrize("case,explicit", HOOK_CASES,
                         ids=[c["ref"] + ("-explicit-preemptible" if e else "") for c, e in HOOK_CASES])
def test_score_reservation_hook(case, explicit):
    """scoreWithNominatedReservation's raw value and its NormalizeReservationScore for the one reservation of the case"""
    orc, _ = oracle_of([U.case_node(case, U.SCORE["gpus"], U.SCORE["rdma"], explicit)], case["strategy"])
    ok, raw, norm, _ = candidate(orc, U.pod_of(case["pod"]), 0, [0],
                                 U.words(case["preemptible"]) if explicit else None)
    orc.close()
    assert ok[0] == 1 and raw[0] == case["want_score"]
    assert norm[0] == (100 if case["want_score"] > 0 else 0)
    if case.get("want_normalized") is not None:
        assert norm[0] == case["want_normalized"]


def test_score_reservation_hook_normalizes_over_rows():
    """two reservations of one node: NormalizeReservationScore is 100 * s / max over the rows that pass"""
    a, b = U.SCORE["cases"][1], U.SCORE["cases"][1]
    spec = U.case_node(a, U.SCORE["gpus"], U.SCORE["rdma"])
    # a second matched reservation holding 25 of the same minor: both remain whole, used is 75 + 25
    spec["rows"].append(U.row("Restricted", U.words({"0": [25, 4, 25]})))
    spec["used"] = {"0": [100, 16, 100]}
    orc, _ = oracle_of([spec], "MostAllocated")
    ok, raw, norm, _ = candidate(orc, U.pod_of(b["pod"]), 0, [0, 1])
    orc.close()
    # row 0 (Default, remained 50, the other's allocatable still counted as used): used' = 100 - 50 = 50, requested
    # 100 of 100 -> MostAllocated 100; row 1 (Restricted, remained 25 < 50) fails FilterReservation
    assert list(ok) == [1, 0] and list(raw) == [100, 0] and list(norm) == [100, 0]


@pytest.mark.parametrize("strategy,pod,cases", U.score_groups(), ids=lambda v: v if isinstance(v, str) else None)
def test_score_reservation_eval_pod(strategy, pod, cases):
    """Oracle.eval_pod on one cluster per (strategy, pod request), each case a node: with its one matched, passing
    reservation nominated, DeviceShare's Score is the ScoreReservation value (scoring.go:72-76), normalized over the
    group's nodes"""
    orc, _ = oracle_of([U.case_node(c, U.SCORE["gpus"], U.SCORE["rdma"]) for c in cases], strategy)
    reasons, scores, _ = orc.eval_pod(U.pod_of(pod))
    orc.close()
    assert not reasons.any()
    assert list(scores[:, abi.KS_SCORE_DEVICESHARE]) == U.normalized([c["want_score"] for c in cases])


def filter_reservation_node(phase):
    f = P["filter_reservation"]
    ph = f[phase]
    return {"gpus": f["gpus"], "used": ph["used_at_call"],
            "rows": [U.row(f["policy"], U.words(f["reserved"]), U.words(ph["assigned_allocated"]), ph["assigned"])]}


def test_filter_reservation_pair():
    f = P["filter_reservation"]
    pod = U.pod_of(f["pod"])
    orc, _ = oracle_of([filter_reservation_node("before")])
    ok, _, _, _ = candidate(orc, pod, 0, [0])
    reasons, _, _ = orc.eval_pod(pod)
    rec, _, _ = orc.assume(pod, 0)
    orc.close()
    assert f["before"]["want"] == "pass" and ok[0] == 1
    assert reasons[0] == 0 and rec["reservation"][0] == 0 and U.minor_list(rec["gpu_minors"][0]) == [1]
    orc, _ = oracle_of([filter_reservation_node("after")])
    ok, _, _, nr = candidate(orc, pod, 0, [0], node_reason=True)
    reasons, _, _ = orc.eval_pod(pod)
    orc.close()
    assert "no reservation(s) to meet the device requirements" in f["after"]["want"] and ok[0] == 0
    # the plain node (plugin.go:316-321: both minors are full once the reservation's allocatable is given back)
    assert nr == abi.KS_R_DEV_INSUFFICIENT and reasons[0] == abi.KS_R_DEV_INSUFFICIENT


@pytest.mark.parametrize("case", P["filter"]["cases"], ids=lambda c: c["ref"])
def test_filter_cases(case):
    pod = U.pod_of(case["pod"])
    orc, _ = oracle_of([U.case_node(case)])
    reasons, _, _ = orc.eval_pod(pod)
    orc.close()
    assert case["want"] == "pass" and reasons[0] == 0
    if case["preemptible"]:
        orc, _ = oracle_of([U.case_node(case, explicit=True)])
        _, _, _, nr = candidate(orc, pod, 0, [], U.words(case["preemptible"]), node_reason=True)
        _, _, _, nr_without = candidate(orc, pod, 0, [], None, node_reason=True)
        orc.close()
        assert nr == 0 and nr_without == abi.KS_R_DEV_INSUFFICIENT


@pytest.mark.parametrize("case", P["reserve"]["cases"], ids=lambda c: c["ref"])
def test_reserve_cases_and_unreserve(case):
    """Reserve's allocation per minor, the reservation it goes into, and Unreserve back to the bytes before"""
    pod = U.pod_of(case["pod"])
    orc, _ = oracle_of([U.case_node(case)])
    before = U.snapshot(orc)
    used0 = [a.copy() for a in orc.read_devices()]
    rd0 = orc.read_reservation_devices().copy()
    rec, cs, na = orc.assume(pod, 0)
    assert rec["status"][0] == abi.KS_S_SCHEDULED
    want = U.words(case["want_allocation"])
    assert U.minor_list(rec["gpu_minors"][0]) == [int(k) for k in case["want_allocation"]]
    used1 = orc.read_devices()
    got = np.zeros(abi.KS_DEV_WORDS, np.int64)
    for q in range(3):
        for k in range(abi.KS_MAX_GPUS):
            got[abi.dev_word("gpu", k, q)] = used1[q][k, 0] - used0[q][k, 0]
    assert np.array_equal(got, want)
    assert (rec["reservation"][0] == 0) == case["want_nominated"]
    grew = orc.read_reservation_devices() - rd0
    if case["want_nominated"]:
        assert np.array_equal(grew[0], want) and orc.read_reservations()[1][0] == 1
    else:
        assert not grew.any() and rec["reservation"][0] == -1
    orc.unreserve(pod, rec, cs, na)
    assert U.snapshot(orc) == before
    orc.close()


def test_unreserve_normal_case():
    u = P["unreserve"]
    pod = U.pod_of(u["pod"])
    orc, _ = oracle_of([{"gpus": u["gpus"], "rdma": u["rdma"], "used": {}, "rows": []}])
    before = U.snapshot(orc)
    rec, cs, na = orc.assume(pod, 0)
    assert U.minor_list(rec["gpu_minors"][0]) == [int(k) for k in u["allocation"]["gpu"]]
    assert U.minor_list(rec["rdma_minors"][0]) == [int(k) for k in u["allocation"]["rdma"]]

    def used_words():
        d = orc.read_devices()
        w = np.zeros(abi.KS_DEV_WORDS, np.int64)
        for k in range(abi.KS_MAX_GPUS):
            for q in range(3):
                w[abi.dev_word("gpu", k, q)] = d[q][k, 0]
        for k in range(abi.KS_MAX_RDMA):
            w[abi.dev_word("rdma", k)] = d[3][k, 0]
        return w

    assert np.array_equal(used_words(), U.words(u["used_before"]["gpu"], u["used_before"]["rdma"]))
    orc.unreserve(pod, rec, cs, na)
    assert np.array_equal(used_words(), U.words(u["used_after"]["gpu"], u["used_after"]["rdma"]))
    assert U.snapshot(orc) == before
    orc.close()


def test_failed_preempt_from_reservation():
    """used 200 on a total of 100 with 100 preemptible: used' = 100, free = max(0, 100 - 100) = 0"""
    f = P["failed_preempt"]
    assert f["want"] == "Insufficient gpu devices"
    pod = U.pod_of(f["pod"])
    orc, _ = oracle_of([U.case_node(f, explicit=True)])
    _, _, _, nr = candidate(orc, pod, 0, [], U.words(f["preemptible"]), node_reason=True)
    orc.close()
    assert nr == abi.KS_R_DEV_INSUFFICIENT
    orc, _ = oracle_of([U.case_node(f)])
    reasons, _, _ = orc.eval_pod(pod)
    orc.close()
    assert reasons[0] == abi.KS_R_DEV_INSUFFICIENT


@pytest.mark.parametrize("sc", U.edge_scenarios(), ids=lambda s: s["name"][:50])
def test_edge_clusters_on_the_oracle(sc):
    """the hand-built edge clusters of the device tests (tests/test_gpu_deviceshare_reservation_golden.py): the oracle
    gives the nomination, verdict and minors worked out by hand in rsv_plugin_util.edge_scenarios"""
    U.run_scenario(lambda cfg, nodes, rs, dev: Oracle(cfg, nodes, reservations=rs, devices=dev), sc)
