"""Builders for the DeviceShare reservation-path golden cases (tests/golden/deviceshare_reservation_plugin.json), shared
by the oracle tests and the device tests.  A node is a dict {gpus, rdma, used, rows}; a row is a reservation on it:
(policy, dev_allocatable words, dev_allocated words, assigned, matched, order).  The pod is in owner class 0, matched
rows are owned by class 0, unmatched ones by class 1."""
import json
import pathlib

import numpy as np

from koordinator_amd import abi
from koordinator_amd.cluster import DeviceTable, NodeTable, PodTable, ReservationTable
from koordinator_amd.config import DeviceShareArgs, SchedulerProfile

G = json.loads((pathlib.Path(__file__).parent / "golden" / "deviceshare_reservation_plugin.json").read_text())
GIB = G["gib"]
POLICY = {"Default": abi.KS_RSV_POLICY_DEFAULT, "Aligned": abi.KS_RSV_POLICY_ALIGNED,
          "Restricted": abi.KS_RSV_POLICY_RESTRICTED}
SCORE = G["score_reservation"]


def words(gpu=None, rdma=None) -> np.ndarray:
    """{minor: [core, GiB, ratio]}, {minor: rdma} -> KS_DEV_WORDS"""
    w = np.zeros(abi.KS_DEV_WORDS, np.int64)
    for k, (core, mem, ratio) in (gpu or {}).items():
        w[abi.dev_word("gpu", int(k), 0)] = core
        w[abi.dev_word("gpu", int(k), 1)] = mem * GIB
        w[abi.dev_word("gpu", int(k), 2)] = ratio
    for k, v in (rdma or {}).items():
        w[abi.dev_word("rdma", int(k))] = v
    return w


ZERO = words()


def row(policy, allocatable, allocated=ZERO, assigned=0, matched=True, order=0):
    return (POLICY.get(policy, policy), allocatable, allocated, assigned, matched, order)


def case_node(c, gpus=None, rdma=None, explicit=False):
    """the node of one transcribed case: its matched reservation (`reserved`, nothing assigned) and, unless explicit,
    its preemptible vector as an unmatched reservation (the fixture's preemptible_mapping)"""
    rows = []
    if c.get("reserved") is not None:
        rows.append(row(c.get("policy", "Default"), words(c["reserved"])))
    if c.get("preemptible") and not explicit:
        rows.append(row("Default", words(c["preemptible"]), words(c["preemptible"]), 1, matched=False))
    return {"gpus": c.get("gpus", gpus), "rdma": c.get("rdma", rdma) or {}, "used": c["used_at_call"], "rows": rows}


def config(strategy="LeastAllocated"):
    return SchedulerProfile(fit=None, loadaware=None, deviceshare=DeviceShareArgs(strategy=strategy),
                            reservation_weight=5000).to_ks_config()


def tables(node_specs):
    """(NodeTable, ReservationTable, DeviceTable, first reservation row of each node)"""
    n = len(node_specs)
    nodes = NodeTable(n)
    nodes.alloc_milli_cpu[:] = 64000
    nodes.alloc_memory[:] = 256 * GIB
    nodes.allowed_pods[:] = 110
    dev = DeviceTable(n)
    dev.flags[:] = abi.KS_DEV_PRESENT
    flat, first = [], []
    for i, ns in enumerate(node_specs):
        for k, (core, mem, ratio) in ns["gpus"].items():
            dev.total_core[int(k), i], dev.total_memory[int(k), i], dev.total_ratio[int(k), i] = core, mem * GIB, ratio
        for k, v in (ns.get("rdma") or {}).items():
            dev.total_rdma[int(k), i] = v
        for k, (core, mem, ratio) in (ns.get("used") or {}).items():
            dev.used_core[int(k), i], dev.used_memory[int(k), i], dev.used_ratio[int(k), i] = core, mem * GIB, ratio
        for k, v in (ns.get("rdma_used") or {}).items():
            dev.used_rdma[int(k), i] = v
        first.append(len(flat))
        flat += [(i,) + r for r in ns["rows"]]
    rs = ReservationTable(len(flat)).hold_devices()
    for j, (i, pol, al, ald, assigned, matched, order) in enumerate(flat):
        rs.node[j] = i
        rs.owner_classes[j] = 1 if matched else 2
        rs.policy[j] = pol
        rs.order[j] = order
        rs.key_mask[j] = 0b11
        rs.allocatable[0, j] = 1000
        rs.assigned[j] = assigned
        rs.dev_allocatable[j] = al
        rs.dev_allocated[j] = ald
    return nodes, rs, dev, first


def pod_of(spec, copies=1) -> PodTable:
    p = PodTable(copies)
    p.req_milli_cpu[:] = 100
    p.nonzero_milli_cpu[:] = 100
    p.nonzero_memory[:] = 200 << 20
    p.rsv_class[:] = 0
    p.gpu_core[:] = spec["core"]
    p.gpu_memory_ratio[:] = spec["ratio"]
    p.flags[:] = abi.KS_POD_GPU_CORE if spec["core"] else 0
    p.rdma[:] = spec.get("rdma", 0)
    return p


def score_groups():
    """TestScoreReservation's cases grouped by (strategy, pod request): each group is one cluster, each case one node"""
    groups = {}
    for c in SCORE["cases"]:
        groups.setdefault((c["strategy"], json.dumps(c["pod"], sort_keys=True)), []).append(c)
    return [(k[0], v[0]["pod"], v) for k, v in groups.items()]


def normalized(raw):
    """DefaultNormalizeScore(100, false): 100 * s / max"""
    m = max(raw)
    return [100 * s // m if m > 0 else s for s in raw]


def snapshot(e):
    """every table a Reserve / Unreserve of a device pod touches, as bytes"""
    parts = list(e.read_devices()) + list(e.read_reservations()) + [e.read_reservation_devices()]
    return [np.ascontiguousarray(a).tobytes() for a in parts]


def minor_list(mask, k=abi.KS_MAX_GPUS):
    return [i for i in range(k) if (int(mask) >> i) & 1]


# ---- hand-built edge clusters (not reference tables): what the code branches on and the tables above lack.  Every GPU
# is 100 / 16Gi / 100.  `want` is for node 0: the nominated reservation (row on the node, -1 = none), the Filter reasons
# and the minors Reserve allocates, worked out from reservation.go:182-271 and nominator.go:134-262 in the comments.

GPU = [100, 16, 100]
HALF = [50, 8, 50]


def edge_scenarios():
    two = {"0": GPU, "1": GPU}
    half = {"core": 50, "ratio": 50, "rdma": 0}
    double = {"core": 200, "ratio": 200, "rdma": 0}
    # A holds half of minor 0, B all of minor 1; on A's view 150 of 200 is requested (LeastAllocated 25), on B's 100
    # of 200 (50): B wins on ScoreReservation though Filter already passes on A (the first matched row)
    ab = [row("Default", words({"0": HALF})), row("Default", words({"1": GPU}))]
    ab_used = {"0": HALF, "1": GPU}
    out = [
        dict(name="higher ScoreReservation nominated, Filter passes on another row", strategy="LeastAllocated", pod=half,
             nodes=[{"gpus": two, "used": ab_used, "rows": ab}], want=dict(nominated=1, reasons=0, gpu=[1])),
        dict(name="MostAllocated turns the same pair round", strategy="MostAllocated", pod=half,
             nodes=[{"gpus": two, "used": ab_used, "rows": ab}], want=dict(nominated=0, reasons=0, gpu=[0])),
        dict(name="equal ScoreReservation: table order", strategy="LeastAllocated", pod=half,
             nodes=[{"gpus": two, "used": {"0": HALF, "1": HALF},
                     "rows": [row("Default", words({"0": HALF})), row("Default", words({"1": HALF}))]}],
             want=dict(nominated=0, reasons=0, gpu=[0])),
        dict(name="order label on the lower-scoring reservation wins", strategy="LeastAllocated", pod=half,
             nodes=[{"gpus": two, "used": ab_used,
                     "rows": [row("Default", words({"0": HALF}), order=1), row("Default", words({"1": GPU}))]}],
             want=dict(nominated=0, reasons=0, gpu=[0])),
        # Restricted requires its minors: one held minor cannot give two instances; the node can (both given back)
        dict(name="Restricted holding part of the request's minors: rejected", strategy="LeastAllocated", pod=double,
             nodes=[{"gpus": two, "used": {"0": GPU}, "rows": [row("Restricted", words({"0": GPU}))]}],
             want=dict(nominated=-1, reasons=0, gpu=[0, 1])),
        # Aligned only prefers them: the second instance comes from the node, the reservation records minor 0 only
        dict(name="Aligned with the same holding: the rest from the node", strategy="LeastAllocated", pod=double,
             nodes=[{"gpus": two, "used": {"0": GPU}, "rows": [row("Aligned", words({"0": GPU}))]}],
             want=dict(nominated=0, reasons=0, gpu=[0, 1])),
    ]
    # 64 unmatched reservations each holding 1 rdma of minor 1 (all of it used by an assigned pod), then at view
    # positions 64 and 65 the matched one (half of GPU 0, whole) and an unmatched one whose assigned pod uses a quarter
    # of GPU 0: the GPU is full, the pod's half fits only with both of them counted (used' = 100 - 50 - 25)
    quarter = {"0": [25, 4, 25]}
    rows = [row("Default", words(rdma={"1": 1}), words(rdma={"1": 1}), 1, matched=False) for _ in range(64)]
    rows += [row("Default", words({"0": HALF})), row("Default", words(quarter), words(quarter), 1, matched=False)]
    out.append(dict(name="reservations at view positions 64 and 65", strategy="LeastAllocated", pod=half,
                    nodes=[{"gpus": {"0": GPU}, "rdma": {"1": 100}, "used": {"0": GPU}, "rdma_used": {"1": 64},
                            "rows": rows}], want=dict(nominated=64, reasons=0, gpu=[0])))
    # the same pod also asking for 40 rdma: 100 - (64 - 64) leaves room only with the 64 unmatched ones given back
    rows2 = list(rows)
    out.append(dict(name="view positions below 64 summed for rdma", strategy="LeastAllocated",
                    pod={"core": 50, "ratio": 50, "rdma": 40},
                    nodes=[{"gpus": {"0": GPU}, "rdma": {"1": 100}, "used": {"0": GPU}, "rdma_used": {"1": 100},
                            "rows": rows2}], want=dict(nominated=64, reasons=0, gpu=[0])))
    return out


def run_scenario(make_engine, sc):
    """eval_pod, assume on node 0 and unreserve of one scenario on an engine (Oracle or Evaluator): returns what it
    did as a dict, after asserting the scenario's `want` and the restore to the bytes before"""
    nodes, rs, dev, first = tables(sc["nodes"])
    e = make_engine(config(sc["strategy"]), nodes, rs, dev)
    try:
        pod = pod_of(sc["pod"])
        want = sc["want"]
        reasons, scores, totals = e.eval_pod(pod)
        assert reasons[0] == want["reasons"], sc["name"]
        before = snapshot(e)
        rd0 = e.read_reservation_devices().copy()
        rec, cs, na = e.assume(pod, 0)
        nom = int(rec["reservation"][0])
        assert nom == (first[0] + want["nominated"] if want["nominated"] >= 0 else -1), (sc["name"], nom)
        assert rec["status"][0] == abi.KS_S_SCHEDULED
        assert minor_list(rec["gpu_minors"][0]) == want["gpu"], sc["name"]
        grew = e.read_reservation_devices() - rd0
        if nom >= 0:
            # the pod's allocation on the nominated reservation's minors becomes part of its allocated
            held = {k for k in range(abi.KS_MAX_GPUS) if rs.dev_allocatable[nom][abi.dev_word("gpu", k, 2)]}
            per = sc["pod"]["ratio"] // max(1, sc["pod"]["ratio"] // 100) if sc["pod"]["ratio"] > 100 else sc["pod"]["ratio"]
            for k in range(abi.KS_MAX_GPUS):
                exp = per if (k in held and k in want["gpu"]) else 0
                assert grew[nom][abi.dev_word("gpu", k, 2)] == exp, (sc["name"], k)
            assert not np.delete(grew, nom, axis=0).any()
        else:
            assert not grew.any()
        after = dict(rec=rec.copy(), reasons=reasons.copy(), scores=scores.copy(), totals=totals.copy(),
                     state=snapshot(e))
        e.unreserve(pod, rec, cs, na)
        assert snapshot(e) == before, sc["name"]
        return after
    finally:
        e.close()
