"""Boundary inputs for the score arithmetic and an exact reference of it (host only; plain Python int / Fraction).

The reference restates the Go formulas and never calls the oracle or the device code:
  least / most term     leastRequestedScore, mostRequestedScore: pkg/scheduler/plugins/loadaware/load_aware.go:388-397,
                        nodenumaresource/least_allocated.go:45-54, nodenumaresource/most_allocated.go:50-62
  weighted mean         resourceAllocationScorer.score: nodenumaresource/scoring.go:206-242 (and the upstream
                        noderesources scorer of the same shape: a resource with capacity 0 is left out, a scalar
                        resource counts only when the pod requests it)
  LoadAware estimate    estimatedUsedByResource: loadaware/estimator/default_estimator.go:73-108, scored on EstimateNode by
                        loadAwareSchedulingScorer: load_aware.go:378-386
  NodeNUMAResource      Amplify: apis/extension/node_resource_amplification.go:170-175; scoreWithAmplifiedCPUs:
                        nodenumaresource/scoring.go:98-114; the amplified request of a cpu-bind pod: plugin.go:503-506

The case builder yields (capacity c, headroom d = h - p, pod request p) triples whose quotient 100 d / c is an integer
or one unit (1/c) off one, at capacities around the device's switch between its f64 and int64 paths (2^43), up to the
validated limit (2^56), and at primes and other capacities without an exact reciprocal.  Case spreads them
over the score terms of a node table laid out in 64-node chunks (one wave each): all below 2^43, all at or above it,
alternating lane by lane, and a partial last chunk.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from koordinator_amd import abi
from koordinator_amd.cluster import CpuState, NodeTable, PodTable, cpu_mask, regular_topology
from koordinator_amd.config import (BATCH_CPU, BATCH_MEMORY, CPU, EPHEMERAL, MEMORY, LoadAwareSchedulingArgs,
                                    NodeNUMAResourceArgs, NodeResourcesFitArgs, SchedulerProfile)

BIG_CAP = 1 << 43  # ks_device.h kBigCap: capacities from here on score in int64
BIG_REQ = 1 << 46  # ks_device.h kBigReq: pod requests from here on score in int64
LIMIT = 1 << 56    # node and pod quantities are validated to [0, 2^56)
SCALAR_NAMES = (BATCH_CPU, BATCH_MEMORY, "example.com/slot2", "example.com/slot3")


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------

def least(requested: int, capacity: int) -> int:
    """leastRequestedScore (load_aware.go:388-397, least_allocated.go:45-54)"""
    if capacity == 0 or requested > capacity:
        return 0
    return (capacity - requested) * 100 // capacity


def most(requested: int, capacity: int) -> int:
    """mostRequestedScore (most_allocated.go:50-62)"""
    if capacity == 0:
        return 0
    return min(requested, capacity) * 100 // capacity


def weighted_mean(terms, scorer) -> int:
    """scoring.go:206-242: terms are (weight, capacity, requested); capacity 0 (or weight 0) leaves the term out"""
    ns = ws = 0
    for w, cap, req in terms:
        if w == 0 or cap == 0:
            continue
        ns += scorer(req, cap) * w
        ws += w
    return ns // ws if ws else 0


def go_round(v: float) -> int:
    """math.Round for v >= 0: half away from zero (Python's round() is half-to-even)"""
    f = math.floor(v)
    return f + 1 if v - f >= 0.5 else f


def estimated_used(req: int, lim: int, sf: int, dflt: int) -> int:
    """estimatedUsedByResource (default_estimator.go:73-108): the f64 expression is Go's, evaluated in f64 here too"""
    if lim > req:
        sf, q = 100, lim
    else:
        q = req
    if q == 0:
        return dflt
    est = go_round(float(q) * float(sf) / 100.0)
    if lim > 0 and est > lim:
        est = lim
    return est


def _fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # Fraction -> float rounds correctly: the IEEE fma


def least_f64(c: int, h: int, p: int, bias: float = 2.0 ** -44) -> int:
    """the device's f64 term (ks_device.h term_least) replayed exactly: trunc(max(fma(100 h - 100 p, fl(1/c), B), 0))"""
    hd, r = (float(h) * 100.0, 1.0 / float(c)) if c else (0.0, 0.0)
    return int(max(_fma(hd - float(p) * 100.0, r, bias), 0.0))


def most_f64(c: int, h: int, p: int, bias: float = 2.0 ** -44) -> int:
    """ks_device.h term_most replayed exactly"""
    hd, r = (float(h) * 100.0, 1.0 / float(c)) if c else (0.0, 0.0)
    return int(min(_fma(float(p) * 100.0 - hd, r, 100.0 + bias), 100.0)) if r != 0.0 else 0


def amplify(x: int, ratio: float) -> int:
    """extension.Amplify (node_resource_amplification.go:170-175); callers apply it for ratio > 1 only"""
    return int(math.ceil(float(x) * ratio)) if ratio > 1 else x


# ---------------------------------------------------------------------------------------------------------------------
# capacities, headrooms, pod requests
# ---------------------------------------------------------------------------------------------------------------------

def is_prime(n: int) -> bool:
    """deterministic Miller-Rabin (the first 12 primes as bases decide every n < 3.3e24)"""
    if n < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for b in bases:
        if n % b == 0:
            return n == b
    s, d = 0, n - 1
    while d % 2 == 0:
        s, d = s + 1, d // 2
    for b in bases:
        x = pow(b, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def next_prime(n: int) -> int:
    while not is_prime(n):
        n += 1
    return n


# primes of 5, 11 and 13 digits; the second 13-digit one lies above 2^43 = 8796093022208
PRIMES = [next_prime(v) for v in (10_000, 65_537, 10 ** 10 + 1, 7 * 10 ** 10, 10 ** 12, 9 * 10 ** 12)]
# 2^43 - 7, 2^44 - 15 (both 1 mod 100) and 2^44 - 17 (99 mod 100): floor(c / 100) and ceil(c / 100) give quotients
# exactly 1/c off an integer, the tightest case of the f64 formula.  It holds at 2^43 - 7; at the other two (which the
# device scores in int64) it is off by one, so a switch moved up to 2^44 shows
CAPS = [1, 2, 3, 7, 100, 101, 999] + PRIMES + [3 << 37, BIG_CAP - 7, BIG_CAP - 3, BIG_CAP - 1, BIG_CAP, BIG_CAP + 1,
                                                 (1 << 44) - 17, (1 << 44) - 15, (1 << 47) + 12345, (1 << 55) + 7, LIMIT - 1]
POD_REQUESTS = [0, 1, 12345, BIG_REQ - 1, BIG_REQ, BIG_REQ + 1, 1 << 55]
KS = (0, 1, 33, 50, 99, 100)


def headrooms(c: int):
    """d in [0, c] with 100 d / c on an integer k, or one unit (1/c) or more just below / above it"""
    out = set()
    for k in KS:
        lo, hi = k * c // 100, -(-k * c // 100)
        out.update(d for d in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if 0 <= d <= c)
    return sorted(out)


def triples(p: int, over: bool = False, caps=None):
    """(c, d, p) the node side can carry: its requested value c - d - p is >= 0.  over adds the overcommitted d < 0
    (requested > capacity), for the terms whose Filter does not read the same column."""
    out = []
    for c in (caps or CAPS):
        ds = list(headrooms(c))
        if over:
            ds += [-1, -c] + ([c - p, c - p - 1] if p > c else [])
        for d in dict.fromkeys(ds):
            if c - d - p >= 0 and c - d - p < LIMIT:
                out.append((c, d, p))
    return out


def all_triples():
    return [t for p in POD_REQUESTS for t in triples(p, over=True)]


# ---------------------------------------------------------------------------------------------------------------------
# evaluation cases
# ---------------------------------------------------------------------------------------------------------------------

N_NODES = 321  # five chunks of 64 and a tail of one node
CHUNK_KINDS = ("small", "big", "mixed", "small", "mixed", "big")


def node_is_big(i: int) -> bool:
    kind = CHUNK_KINDS[i // 64]
    return kind == "big" or (kind == "mixed" and i % 2 == 1)


@dataclass
class Spec:
    """one evaluation case: the profile, the pod and how the triples are dealt to the nodes' terms"""
    strategy: str = "LeastAllocated"
    fit_w: tuple = (1, 1)          # cpu, memory
    eph_w: int = 0
    nsc: int = 0                   # scalar slots with a weight (0, 2, 4)
    pod_scalars: bool = False      # the pod requests the scalar slots
    la_w: tuple = (1, 1)
    prod_usage: bool = False
    prod_pod: bool = False
    sf: tuple = (85, 70)
    la_mode: str = "dflt"          # "dflt": request = limit = 0; "lim": limit > request; "req": limit = 0
    pa: int = 12345                # the pod's cpu-like requests (non-zero cpu, estimate cpu, even scalar slots)
    pb: int = 1                    # the pod's memory-like requests
    pe: int = 0                    # ephemeral-storage and scalar requests (Filter-checked: kept small)
    numa: Optional[float] = None   # NodeNUMAResource on with this amplification ratio (None = off)
    numa_strategy: str = "LeastAllocated"
    bind: bool = False             # a cpu-bind pod (NodeNUMAResource cases)
    plugin_w: tuple = (1, 1, 1)    # Fit, LoadAware, NodeNUMAResource
    rot: int = 0                   # rotates which triple lands on which node
    balanced: bool = False
    n: int = N_NODES

    def name(self) -> str:
        s = f"{self.strategy[:5]}-f{self.fit_w[0]}.{self.fit_w[1]}.{self.eph_w}-sc{self.nsc}{'r' if self.pod_scalars else ''}" \
            f"-la{self.la_w[0]}.{self.la_w[1]}{'P' if self.prod_usage else ''}{'p' if self.prod_pod else ''}-{self.la_mode}" \
            f"-pa{self.pa:#x}-pb{self.pb:#x}-pe{self.pe}"
        if self.numa is not None:
            s += f"-numa{self.numa}{'b' if self.bind else ''}{self.numa_strategy[:1]}"
        return s

    def profile(self, quota=None, batch_pods=0, candidates=0) -> SchedulerProfile:
        res = {CPU: self.fit_w[0], MEMORY: self.fit_w[1]}
        if self.eph_w:
            res[EPHEMERAL] = self.eph_w
        for k in range(self.nsc):
            res[SCALAR_NAMES[k]] = (1, 3, 2, 5)[k]
        la = LoadAwareSchedulingArgs(score_according_prod_usage=self.prod_usage,
                                     resource_weights={CPU: self.la_w[0], MEMORY: self.la_w[1]},
                                     estimated_scaling_factors={CPU: self.sf[0], MEMORY: self.sf[1]})
        p = SchedulerProfile(fit=NodeResourcesFitArgs(strategy=self.strategy, resources=res), fit_weight=self.plugin_w[0],
                             loadaware=la, loadaware_weight=self.plugin_w[1], scalar_slots=SCALAR_NAMES, quota=quota,
                             batch_pods=batch_pods, candidates=candidates)
        if self.numa is not None:
            p.numa = NodeNUMAResourceArgs(strategy=self.numa_strategy, resources={CPU: 1, MEMORY: 3})
            p.numa_weight = self.plugin_w[2]
        if self.balanced:
            from koordinator_amd.config import NodeResourcesBalancedAllocationArgs

            p.balanced = NodeResourcesBalancedAllocationArgs()
        return p


def la_columns(p: int, mode: str, sf: int):
    """(la_req, la_lim, la_dflt) whose estimate is p ("dflt", "lim") or the nearest value the mode can give ("req")"""
    if mode == "dflt" or p == 0:
        return 0, 0, p
    if mode == "lim":
        return p // 2, p, 250
    return min(-(-p * 100 // sf), LIMIT - 1), 0, 250


class Case:
    """A node table, one pod, the profile, the CPU state of a cpu-bind case and the reference's expected columns."""

    def __init__(self, spec: Spec):
        self.spec = s = spec
        n = s.n
        self.profile = s.profile()
        self.cfg = self.profile.to_ks_config()
        pod = self.pod = PodTable(1)
        numa = s.numa is not None
        pa, pb = s.pa, s.pb
        if s.bind:
            assert numa and pa % 1000 == 0 and 0 < pa <= 32000
        pod.nonzero_milli_cpu[0], pod.nonzero_memory[0] = pa, pb
        if numa:
            pod.req_milli_cpu[0], pod.req_memory[0] = pa, pb  # the Requested columns carry the boundary (d >= 0 only)
        pod.req_ephemeral[0] = s.pe if s.eph_w else 0
        if s.pod_scalars:
            for k in range(s.nsc):
                pod.req_scalar[k][0] = s.pe + k if s.pe else 0
            if s.pe and s.nsc:
                pod.flags[0] |= abi.KS_POD_SCALAR_KEYS
        if s.prod_pod:
            pod.flags[0] |= abi.KS_POD_PROD
        if s.bind:
            pod.flags[0] |= abi.KS_POD_CPU_BIND
            pod.cpu_bind[0] = abi.KS_CPU_BIND_SPREAD_BY_PCPUS
        pod.la_req_cpu[0], pod.la_lim_cpu[0], pod.la_dflt_cpu[0] = la_columns(pa, s.la_mode, s.sf[0])
        pod.la_req_memory[0], pod.la_lim_memory[0], pod.la_dflt_memory[0] = la_columns(pb, s.la_mode, s.sf[1])
        self.est = (estimated_used(int(pod.la_req_cpu[0]), int(pod.la_lim_cpu[0]), s.sf[0], int(pod.la_dflt_cpu[0])),
                    estimated_used(int(pod.la_req_memory[0]), int(pod.la_lim_memory[0]), s.sf[1], int(pod.la_dflt_memory[0])))

        t = self.nodes = NodeTable(n)
        t.allowed_pods[:] = 110
        t.la_flags[:] = abi.KS_LA_HAS_METRIC  # scored; no usage threshold is set, so the LoadAware Filter passes
        self.cpu_state = None
        a_cpus = np.zeros(n, np.int64)
        if numa:
            t.numa_cpu_amplification[:] = s.numa
            a_cpus = np.array([(0, 24, 7, 3)[i % 4] for i in range(n)], np.int64)
        # the term slots: (capacity column, requested column, pod request, overcommit allowed)
        over_fit = not numa  # with NodeNUMAResource on, non-zero requested == requested, which the Filter reads
        slots = [("alloc_milli_cpu", "nonzero_milli_cpu", pa, over_fit), ("alloc_memory", "nonzero_memory", pb, over_fit),
                 ("la_alloc_milli_cpu", "la_term_milli_cpu", self.est[0], True),
                 ("la_alloc_memory", "la_term_memory", self.est[1], True),
                 ("alloc_ephemeral", "req_ephemeral", int(pod.req_ephemeral[0]), False)]
        for k in range(s.nsc):
            slots.append((("alloc_scalar", k), ("req_scalar", k), int(pod.req_scalar[k][0]), False))
        lists = {}

        def tri(p, over, big):
            key = (p, over, big)
            if key not in lists:
                caps = [c for c in CAPS if (c >= BIG_CAP) == big]
                lists[key] = triples(p, over, caps)
            return lists[key]

        def put(col, i, v):
            if isinstance(col, tuple):
                getattr(t, col[0])[col[1]][i] = v
            else:
                getattr(t, col)[i] = v

        self.turned_big = np.zeros(n, bool)  # dealt as small, but only a capacity >= 2^43 holds the pod's request
        n_big = sum(node_is_big(i) for i in range(n))
        cls_idx = [0, 0]
        self.used = []  # (c, d, p) per (node, slot), None where the term has no capacity
        for i in range(n):
            big = node_is_big(i)
            j = cls_idx[big]
            cls_idx[big] += 1
            n_cls = n_big if big else n - n_big
            row = []
            for si, (ccol, rcol, p, over) in enumerate(slots):
                # a big node needs one capacity at or above 2^43: its first two slots; the others mix both ranges
                lst = tri(p, over, big if (si < 2 or not big) else (j + si) % 2 == 0)
                zero = i % 16 == 5 and (i // 16) % len(slots) == si
                if numa and si < 2:
                    zero = False  # a pod with a cpu / memory request does not fit a node without that capacity
                if si >= 4 and p != 0:
                    zero = False
                if not lst and not over and p != 0:
                    lst = tri(p, over, True)  # no capacity below 2^43 holds this request: the node turns big
                    self.turned_big[i] = self.turned_big[i] or not big
                if zero or not lst:
                    # the kNoCap case: capacity 0 (only where the pod's request keeps the node feasible)
                    put(ccol, i, 0)
                    put(rcol, i, (i * 37) % 1000 if not (si < 2 and numa) and si < 4 else 0)
                    row.append(None)
                    continue
                c, d, _ = lst[(j + si * n_cls + s.rot) % len(lst)]
                put(ccol, i, c)
                put(rcol, i, c - d - p)
                row.append((c, d, p))
            self.used.append(row)
            # the prod term of LoadAware: another headroom of the same capacity
            for ccol, rcol, prcol, p in (("la_alloc_milli_cpu", "la_term_milli_cpu", "la_prod_term_milli_cpu", self.est[0]),
                                         ("la_alloc_memory", "la_term_memory", "la_prod_term_memory", self.est[1])):
                c = int(getattr(t, ccol)[i])
                hs = [d for d in headrooms(c) if c - d - p >= 0] if c else []
                getattr(t, prcol)[i] = (c - hs[(i + s.rot) % len(hs)] - p) if hs else int(getattr(t, rcol)[i])
            if numa:
                # Requested: the boundary sits on the amplified value, requested - A + Amplify(A) (scoring.go:98-114);
                # A (the cpuset-held milli-CPUs) is kept only where requested >= A, as the Filter's adjustment needs
                c, amp_p = int(t.alloc_milli_cpu[i]), amplify(pa, s.numa) if s.bind else pa
                d = int(t.alloc_milli_cpu[i] - t.nonzero_milli_cpu[i]) - pa
                A = int(a_cpus[i]) * 1000
                req = c - d - amp_p - (amplify(A, s.numa) - A)
                if req < A:
                    A, a_cpus[i] = 0, 0
                    req = c - d - amp_p
                if req < 0:  # the amplified request no longer fits under this headroom: keep the plain boundary
                    req = c - d - pa if not s.bind else max(c - amp_p, 0)
                    if s.bind and c < amp_p:
                        raise AssertionError("capacity below the amplified request")
                t.req_milli_cpu[i] = t.nonzero_milli_cpu[i] = req
                t.req_memory[i] = t.nonzero_memory[i]
        if numa:
            t.numa_cpuset_cpus[:] = a_cpus
            if s.bind:
                cs = self.cpu_state = CpuState(n, [regular_topology(2, 1, 16, 2)])
                cs.topology[:] = 0
                for i in range(n):
                    cs.allocated[i] = cpu_mask(range(int(a_cpus[i])))
        self.want = reference_eval(self.cfg, t, pod, s)

    def tables(self) -> dict:
        return {"cpu_state": self.cpu_state.copy()} if self.cpu_state is not None else {}

    def big_nodes(self) -> np.ndarray:
        """per node: a score-term capacity of the built table is >= 2^43 (what prep_nodes_kernel flags kNodeBigCap)"""
        t = self.nodes
        big = np.zeros(t.n, bool)
        for col in (t.alloc_milli_cpu, t.alloc_memory, t.alloc_ephemeral, t.la_alloc_milli_cpu, t.la_alloc_memory,
                    *t.alloc_scalar):
            big |= np.asarray(col) >= BIG_CAP
        return big


def reference_eval(cfg, t: NodeTable, pod: PodTable, s: Spec, i_pod: int = 0) -> dict:
    """Fit, LoadAware, NodeNUMAResource and the weighted total of pod i_pod on every node of t (all assumed feasible,
    every node with a fresh NodeMetric, topology-policy None), in Python integers."""
    g = lambda a: int(a[i_pod])  # noqa: E731
    sc_fit = most if s.strategy == "MostAllocated" else least
    sc_numa = most if s.numa_strategy == "MostAllocated" else least
    est = (estimated_used(g(pod.la_req_cpu), g(pod.la_lim_cpu), s.sf[0], g(pod.la_dflt_cpu)),
           estimated_used(g(pod.la_req_memory), g(pod.la_lim_memory), s.sf[1], g(pod.la_dflt_memory)))
    prod = bool(g(pod.flags) & abi.KS_POD_PROD) and s.prod_usage
    bind = bool(g(pod.flags) & abi.KS_POD_CPU_BIND)
    psc = [int(pod.req_scalar[k][i_pod]) for k in range(abi.KS_MAX_SCALARS)]
    reqzero = g(pod.req_milli_cpu) == 0 and g(pod.req_memory) == 0 and g(pod.req_ephemeral) == 0 and not any(psc)
    fw_sc = [int(cfg.fit.weight_scalar[k]) for k in range(abi.KS_MAX_SCALARS)]
    out = {k: np.zeros(t.n, np.int64) for k in ("fit", "la", "numa", "total")}
    for i in range(t.n):
        terms = [(s.fit_w[0], int(t.alloc_milli_cpu[i]), int(t.nonzero_milli_cpu[i]) + g(pod.nonzero_milli_cpu)),
                 (s.fit_w[1], int(t.alloc_memory[i]), int(t.nonzero_memory[i]) + g(pod.nonzero_memory)),
                 (s.eph_w, int(t.alloc_ephemeral[i]), int(t.req_ephemeral[i]) + g(pod.req_ephemeral))]
        for k in range(abi.KS_MAX_SCALARS):
            if psc[k] != 0:  # a scalar resource counts only when the pod requests it
                terms.append((fw_sc[k], int(t.alloc_scalar[k][i]), int(t.req_scalar[k][i]) + psc[k]))
        fit = weighted_mean(terms, sc_fit)
        tc = int((t.la_prod_term_milli_cpu if prod else t.la_term_milli_cpu)[i])
        tm = int((t.la_prod_term_memory if prod else t.la_term_memory)[i])
        # loadAwareSchedulingScorer keeps a resource without capacity in the weight sum (its score is 0)
        la = (least(tc + est[0], int(t.la_alloc_milli_cpu[i])) * s.la_w[0] +
              least(tm + est[1], int(t.la_alloc_memory[i])) * s.la_w[1]) // (s.la_w[0] + s.la_w[1])
        numa = 0
        if s.numa is not None and not reqzero:
            ratio = float(t.numa_cpu_amplification[i])
            rq, pc = int(t.req_milli_cpu[i]), g(pod.req_milli_cpu)
            if pc != 0 and ratio > 1:
                A = int(t.numa_cpuset_cpus[i]) * 1000
                rq = rq - A + amplify(A, ratio)
                if bind:
                    pc = amplify(pc, ratio)
            numa = weighted_mean([(int(cfg.numa.weight_cpu), int(t.alloc_milli_cpu[i]), rq + pc),
                                  (int(cfg.numa.weight_memory), int(t.alloc_memory[i]), int(t.req_memory[i]) + g(pod.req_memory))],
                                 sc_numa)
        out["fit"][i], out["la"][i], out["numa"][i] = fit, la, numa
        out["total"][i] = fit * s.plugin_w[0] + la * s.plugin_w[1] + (numa * s.plugin_w[2] if s.numa is not None else 0)
    return out


def matrix():
    """The evaluation cases of the CPU test and of the device's ks_eval_pod test."""
    out = []
    rot = 0

    def add(**kw):
        nonlocal rot
        out.append(Spec(rot=rot, **kw))
        rot += 53

    # every pod request pair, both strategies, the Fit weights in turn
    fit_ws = [(1, 1), (1, 100), (100, 1), (3, 7)]
    pairs = [(0, 0), (1, 12345), (12345, 1), (BIG_REQ - 1, 12345), (12345, BIG_REQ - 1), (BIG_REQ, 1), (1, BIG_REQ),
             (BIG_REQ + 1, BIG_REQ - 1), (1 << 55, 12345), (12345, 1 << 55), (BIG_REQ - 1, BIG_REQ - 1)]
    k = 0
    for strategy in ("LeastAllocated", "MostAllocated"):
        for pa, pb in pairs:
            for mode in (("dflt", "lim", "req") if pa < (1 << 55) and pb < (1 << 55) else ("dflt", "lim")):
                add(strategy=strategy, fit_w=fit_ws[k % 4], pa=pa, pb=pb, la_mode=mode, la_w=((1, 1), (100, 1))[k % 2],
                    prod_usage=k % 3 != 0, prod_pod=k % 4 < 2, sf=((85, 70), (70, 85), (100, 1))[k % 3],
                    plugin_w=((1, 1, 1), (2, 3, 1))[k % 2])
                k += 1
    # ephemeral-storage and 0 / 2 / 4 scalar slots, with pods that do and do not request them
    for strategy in ("LeastAllocated", "MostAllocated"):
        for nsc in (0, 2, 4):
            for pod_scalars in (False, True):
                for pe in (1, 12345):
                    for pa, pb in ((12345, 1), (BIG_REQ, 12345)):
                        add(strategy=strategy, fit_w=fit_ws[k % 4], eph_w=(1, 2)[k % 2], nsc=nsc, pod_scalars=pod_scalars,
                            pe=pe, pa=pa, pb=pb, prod_usage=True, prod_pod=k % 2 == 0)
                        k += 1
    # NodeNUMAResource, topology-policy None: ratios 1.0, 1.5 (24000 x 1.5 is an exact integer), 1.0000001, 1.25
    for ratio in (1.0, 1.5, 1.0000001, 1.25):
        for numa_strategy in ("LeastAllocated", "MostAllocated"):
            for bind, pa, pb in ((False, 12345, 1), (False, 1, 12345), (True, 3000, 12345), (False, BIG_REQ, BIG_REQ - 1),
                                 (False, 0, 12345)):
                add(numa=ratio, numa_strategy=numa_strategy, bind=bind, pa=pa, pb=pb, strategy=("LeastAllocated", "MostAllocated")[k % 2],
                    plugin_w=((1, 1, 1), (1, 2, 3))[k % 2])
                k += 1
    return out


def reciprocal_directions():
    """the capacities below 2^43 whose f64 reciprocal is rounded down / up (exact ones in neither)"""
    down = [c for c in CAPS if c < BIG_CAP and Fraction(1.0 / float(c)) < Fraction(1, c)]
    up = [c for c in CAPS if c < BIG_CAP and Fraction(1.0 / float(c)) > Fraction(1, c)]
    return down, up


# ---------------------------------------------------------------------------------------------------------------------
# queues whose Reserves walk the nodes' quotients across integer boundaries
# ---------------------------------------------------------------------------------------------------------------------

Q_SMALL = [7, 101, 999, PRIMES[0], PRIMES[2], PRIMES[4], 3 << 37, BIG_CAP - 3, BIG_CAP - 1]
Q_BIG = [BIG_CAP, BIG_CAP + 1, PRIMES[5], (1 << 47) + 12345, (1 << 55) + 7, LIMIT - 1]
RESULT_COLS = ("node", "status", "score", "reservation", "gpu_minors", "rdma_minors")


def queue_nodes(n: int = 57, numa: bool = False) -> NodeTable:
    """Two nodes in three with every capacity below 2^43, the third with capacities at or above it; the requested
    values start on k c / 100 boundaries; one LoadAware and one Fit term without capacity; 4 pods per node at most, so
    the queue spreads over the nodes and comes back to the slots it touched."""
    t = NodeTable(n)
    t.allowed_pods[:] = 4
    t.la_flags[:] = abi.KS_LA_HAS_METRIC
    cols = (("alloc_milli_cpu", "nonzero_milli_cpu"), ("alloc_memory", "nonzero_memory"),
            ("la_alloc_milli_cpu", "la_term_milli_cpu"), ("la_alloc_memory", "la_term_memory"))
    for i in range(n):
        big = i % 3 == 2
        for si, (ccol, rcol) in enumerate(cols):
            lst = Q_BIG if big and (si == i // 3 % 4 or i % 2) else Q_SMALL
            c = lst[(i // 3 + 2 * si) % len(lst)]
            getattr(t, ccol)[i] = c
            getattr(t, rcol)[i] = (0, 1, 33, 50)[(i + si) % 4] * c // 100
        t.alloc_scalar[0][i] = Q_SMALL[i % len(Q_SMALL)] if not big else Q_BIG[i % len(Q_BIG)]
        t.alloc_scalar[1][i] = 1 << 20
        t.alloc_ephemeral[i] = 1 << 40
    t.la_prod_term_milli_cpu[:] = t.la_term_milli_cpu // 2
    t.la_prod_term_memory[:] = t.la_term_memory // 3
    t.la_alloc_memory[4] = 0
    t.la_term_memory[4] = t.la_prod_term_memory[4] = 0
    t.alloc_memory[9] = 0
    t.nonzero_memory[9] = 0
    if numa:
        # NodeNUMAResource scores Requested: it starts where the non-zero requested does; amplified CPUs, no cpuset pods
        t.req_milli_cpu[:] = t.nonzero_milli_cpu
        t.req_memory[:] = t.nonzero_memory
        t.numa_cpu_amplification[:] = np.array([1.0, 1.5, 1.0000001, 1.25])[np.arange(n) % 4]
    return t


def queue_pods(p: int, shift: int = 0, quotas: int = 0, numa: bool = False) -> PodTable:
    """Non-zero requests and LoadAware estimates of c // 100, ceil(c / 100) and 1 for the nodes' capacities c; the
    Requested columns stay 0 (the Filter passes however large the request) unless NodeNUMAResource scores them; the
    pod in mid-queue requests (2^55 + 7) // 100 >= 2^46 bytes."""
    t = PodTable(p)
    caps = Q_SMALL + Q_BIG[:4]  # c // 100 < 2^46 for all of these
    for j in range(p):
        def val(o):
            c = caps[(j + shift + o) % len(caps)]
            return (c // 100, -(-c // 100), 1)[(j + o) % 3]
        t.nonzero_milli_cpu[j], t.nonzero_memory[j] = val(0), val(5)
        if j == p // 2:
            t.nonzero_memory[j] = ((1 << 55) + 7) // 100
        ec, em = val(3), val(7)
        if j % 2:
            t.flags[j] |= abi.KS_POD_PROD
            t.la_dflt_cpu[j], t.la_dflt_memory[j] = ec, em
        else:
            t.la_lim_cpu[j], t.la_req_cpu[j], t.la_dflt_cpu[j] = ec, ec // 2, 250
            t.la_lim_memory[j], t.la_req_memory[j], t.la_dflt_memory[j] = em, em // 2, 200 << 20
        if j % 5 == 0:
            t.req_scalar[0][j] = 1
            t.flags[j] |= abi.KS_POD_SCALAR_KEYS
        if numa:
            t.req_milli_cpu[j], t.req_memory[j] = t.nonzero_milli_cpu[j], t.nonzero_memory[j]
        if quotas:
            from koordinator_amd import synth

            t.quota[j] = j % quotas
            t.quota_req[synth.QDIM_CPU][j] = int(t.nonzero_milli_cpu[j]) % 100_000 + 1
            t.quota_req[synth.QDIM_MEMORY][j] = int(t.nonzero_memory[j]) % (1 << 30) + 1
            t.quota_mask[j] = (1 << synth.QDIM_CPU) | (1 << synth.QDIM_MEMORY)
    return t


def queue_profile(quota: bool = False, strategy: str = "LeastAllocated", batch_pods: int = 0, candidates: int = 0,
                  balanced: bool = False, numa: bool = False) -> SchedulerProfile:
    from koordinator_amd.config import ElasticQuotaArgs

    s = Spec(strategy=strategy, nsc=2, prod_usage=True, numa=1.5 if numa else None, balanced=balanced)
    return s.profile(quota=ElasticQuotaArgs() if quota else None, batch_pods=batch_pods, candidates=candidates)


def queue_quotas(pods: PodTable, q: int = 3):
    from koordinator_amd import synth

    return synth.make_quotas(pods, q, np.random.Generator(np.random.PCG64(5)), admit_frac=0.8)


def check_queues(runtime, oracle_mod, prof, nodes, queues, quotas=None, vshards: int = 1, label: str = ""):
    """Schedules the queues one after the other on one device context and one oracle; result columns, node state and
    quota `used` must be equal after each.  Returns the device's stats after the first queue and the oracle's results."""
    cfg = prof.to_ks_config()
    kw = {"quotas": quotas.copy()} if quotas is not None else {}
    ev = runtime.Evaluator(cfg, nodes.copy(), **kw)
    orc = oracle_mod.Oracle(cfg, nodes.copy(), nthreads=2, **kw)
    stats, wants = None, []
    try:
        if vshards > 1:
            ev.shard(1, 0, None, vshards)
        for qi, pods in enumerate(queues):
            tag = f"{label} queue {qi}"
            want, got = orc.schedule(pods), ev.schedule(pods)
            for k in RESULT_COLS:
                bad = np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0]
                assert not len(bad), f"{tag}: {k} differs at {len(bad)} pods; pod {int(bad[0])}: device " \
                                     f"{got[k][bad[0]]} (node {got['node'][bad[0]]}), oracle {want[k][bad[0]]} (node {want['node'][bad[0]]})"
            gs, ws = ev.read_nodes().as_dict(), orc.read_nodes().as_dict()
            for k in ws:
                assert np.array_equal(gs[k], ws[k]), f"{tag}: node state {k}"
            if quotas is not None:
                assert np.array_equal(ev.read_quota_used(), orc.read_quota_used()), f"{tag}: quota used"
            if stats is None:
                stats = ev.stats()
            wants.append(want)
    finally:
        ev.close()
        orc.close()
    return stats, wants


def run_reserve_walk(runtime, oracle_mod, quota: bool, label: str = "", **prof_kw):
    """The two-queue Reserve walk of tests/test_gpu_score_edges.py (also the body of its child processes)."""
    numa = bool(prof_kw.get("numa"))
    vshards = prof_kw.pop("vshards", 1)
    nodes = queue_nodes(57, numa)
    queues = [queue_pods(130, 0, 3 if quota else 0, numa), queue_pods(64, 4, 3 if quota else 0, numa)]
    q = queue_quotas(queue_pods(194, 0, 3, numa)) if quota else None  # limits sized on both queues' demand
    stats, wants = check_queues(runtime, oracle_mod, queue_profile(quota=quota, **prof_kw), nodes, queues, q, vshards, label)
    placed = np.asarray(wants[0]["node"])[np.asarray(wants[0]["status"]) == abi.KS_S_SCHEDULED]
    assert len(placed) > 57 >= len(np.unique(placed)), "the queue must come back to nodes it already reserved on"
    return stats, wants


# ---------------------------------------------------------------------------------------------------------------------
# DeviceShare (always the int64 path, ks_dev.h): GPU memory totals that are prime or next to the validated limit
# ---------------------------------------------------------------------------------------------------------------------

DEV_TOTALS = [PRIMES[2], PRIMES[4], BIG_CAP - 1, BIG_CAP, BIG_CAP + 1, PRIMES[5], (1 << 55) + 7, LIMIT - 1]


def device_workload(n: int = 48, p: int = 60):
    """(nodes, devices, pods): two GPUs per node whose gpu-memory totals are DEV_TOTALS, used up to k % of them on
    k c / 100 boundaries; pods ask for c // 100, ceil(c / 100) or 1 bytes of gpu-memory, or for a gpu-memory-ratio."""
    from koordinator_amd.cluster import DeviceTable

    nodes = queue_nodes(n)
    nodes.allowed_pods[:] = 110
    d = DeviceTable(n)
    d.flags[:] = abi.KS_DEV_PRESENT
    for i in range(n):
        for k in range(2):
            c = DEV_TOTALS[(i + 3 * k) % len(DEV_TOTALS)]
            used = (0, 1, 33, 50)[(i + k) % 4]
            d.total_core[k, i], d.total_ratio[k, i], d.total_memory[k, i] = 100, 100, c
            d.used_core[k, i], d.used_ratio[k, i], d.used_memory[k, i] = used, used, used * c // 100
    pods = queue_pods(p)
    for j in range(p):
        c = DEV_TOTALS[j % len(DEV_TOTALS)]
        if j % 3 == 2:
            pods.gpu_core[j] = pods.gpu_memory_ratio[j] = (1, 33, 50, 99)[j // 3 % 4]
            pods.flags[j] |= abi.KS_POD_GPU_CORE
        else:
            pods.gpu_memory[j] = (c // 100, -(-c // 100), 1)[j % 3 + (j // 3) % 2]
            pods.flags[j] |= abi.KS_POD_GPU_MEMORY
    return nodes, d, pods


def device_profile(strategy: str = "LeastAllocated") -> SchedulerProfile:
    from koordinator_amd.config import GPU_CORE, GPU_MEMORY, GPU_MEMORY_RATIO, DeviceShareArgs

    prof = queue_profile()
    prof.deviceshare = DeviceShareArgs(strategy=strategy, resources={GPU_CORE: 1, GPU_MEMORY: 3, GPU_MEMORY_RATIO: 2})
    return prof


# ---------------------------------------------------------------------------------------------------------------------
# Reservation (ks_rsv.h rsv_score) and the NUMA topology policy scorer (ks_numa.h numa_res_score): always int64
# ---------------------------------------------------------------------------------------------------------------------

RSV_TOTALS = [(1 << 55) + 7, BIG_CAP - 1, BIG_CAP, BIG_CAP + 1, PRIMES[4], PRIMES[5]]
NUMA_LIMIT = 1 << 50  # ks_load_numa_nodes accepts per-NUMA quantities up to this value
NUMA_TOTALS = [NUMA_LIMIT, NUMA_LIMIT - 1, NUMA_LIMIT - 75, NUMA_LIMIT - 77, next_prime(NUMA_LIMIT - 1000)]


def reservation_workload(n: int = 40, r: int = 60, p: int = 64):
    """(nodes, reservations, pods): reservations whose memory allocatable is RSV_TOTALS, allocated up to k % of it on
    k c / 100 boundaries; the pods of their owner classes ask for c // 100, ceil(c / 100) or 1 bytes, so the
    MostAllocated quotient (request + allocated) / allocatable of scoreReservation sits on or next to an integer.
    The reserve pods and their assigned pods are in the nodes' NodeInfo, as the scheduler cache holds them."""
    from koordinator_amd.cluster import ReservationTable

    nodes = NodeTable(n)
    nodes.allowed_pods[:] = 110
    nodes.alloc_milli_cpu[:] = 10 ** 9
    nodes.alloc_memory[:] = LIMIT - 1
    nodes.la_flags[:] = abi.KS_LA_HAS_METRIC
    nodes.la_alloc_milli_cpu[:] = nodes.alloc_milli_cpu
    nodes.la_alloc_memory[:] = nodes.alloc_memory
    rs = ReservationTable(r)
    for i in range(r):
        c = RSV_TOTALS[i % len(RSV_TOTALS)] if i < 48 else RSV_TOTALS[1 + i % 5]
        k = (0, 1, 33, 50)[i // 2 % 4]
        if i < 48:
            rs.node[i] = (i * 7) % n
        else:  # the last dozen share a node with an earlier reservation, where both fit the node's range
            rs.node[i] = next(nd for nd in range(i % 6, n) if 0 < nodes.req_memory[nd] < LIMIT - 1 - 2 * c)
        rs.owner_classes[i] = np.uint64(1) << np.uint64(i % 4)
        rs.policy[i] = (abi.KS_RSV_POLICY_DEFAULT, abi.KS_RSV_POLICY_ALIGNED, abi.KS_RSV_POLICY_RESTRICTED)[i % 3]
        rs.key_mask[i] = 0b11
        rs.allocatable[0][i], rs.allocatable[1][i] = 64000, c
        rs.allocated[0][i], rs.allocated[1][i] = (k * 640, k * c // 100)
        rs.assigned[i] = 1 if k else 0
        nd = int(rs.node[i])
        nodes.req_milli_cpu[nd] += 64000 + k * 640
        nodes.req_memory[nd] += c + k * c // 100
        nodes.pod_count[nd] += 1 + (1 if k else 0)
    nodes.nonzero_milli_cpu[:] = nodes.req_milli_cpu
    nodes.nonzero_memory[:] = nodes.req_memory
    assert int(nodes.req_memory.max()) < LIMIT - 1
    pods = PodTable(p)
    for j in range(p):
        c = RSV_TOTALS[(j // 4) % len(RSV_TOTALS)]
        pods.req_milli_cpu[j] = pods.nonzero_milli_cpu[j] = (640, 641, 1000)[j % 3]
        pods.req_memory[j] = pods.nonzero_memory[j] = (c // 100, -(-c // 100), 1)[j % 3]
        pods.rsv_class[j] = j % 4 if j % 8 != 7 else -1
        pods.la_dflt_cpu[j], pods.la_dflt_memory[j] = 250, 200 << 20
    return nodes, rs, pods


def reservation_profile() -> SchedulerProfile:
    return SchedulerProfile(fit=NodeResourcesFitArgs(resources={CPU: 1, MEMORY: 1}), reservation_weight=5000)


def numa_policy_workload(n: int = 48, p: int = 64):
    """(nodes, NUMA nodes, pods): every node has a NUMA topology policy and one or two NUMA nodes whose cpu and memory
    are NUMA_TOTALS (the loader's limit 2^50, just under it, a prime), used up to k % on k c / 100 boundaries; pods ask
    for c // 100, ceil(c / 100) or 1."""
    from koordinator_amd.cluster import NumaNodes

    nodes = NodeTable(n)
    nodes.allowed_pods[:] = 110
    nodes.la_flags[:] = abi.KS_LA_HAS_METRIC
    nn = NumaNodes(n)
    for i in range(n):
        nodes.numa_flags[i] = (abi.KS_NUMA_POLICY_BEST_EFFORT, abi.KS_NUMA_POLICY_RESTRICTED,
                               abi.KS_NUMA_POLICY_SINGLE_NUMA_NODE)[i % 3] << abi.KS_NUMA_POLICY_SHIFT
        cnt = 1 + i % 2
        nn.count[i] = cnt
        for j in range(cnt):
            cc, cm = NUMA_TOTALS[(i + j) % len(NUMA_TOTALS)], NUMA_TOTALS[(i + 2 * j + 1) % len(NUMA_TOTALS)]
            k = (0, 1, 33, 50)[(i // 2 + j) % 4]
            nn.alloc_cpu[i, j], nn.alloc_memory[i, j] = cc, cm
            nn.used_cpu[i, j], nn.used_memory[i, j] = k * cc // 100, k * cm // 100
            nn.used_present[i, j] = 1 if k else 0
        nodes.alloc_milli_cpu[i], nodes.alloc_memory[i] = int(nn.alloc_cpu[i].sum()), int(nn.alloc_memory[i].sum())
        nodes.req_milli_cpu[i], nodes.req_memory[i] = int(nn.used_cpu[i].sum()), int(nn.used_memory[i].sum())
    nodes.nonzero_milli_cpu[:] = nodes.req_milli_cpu
    nodes.nonzero_memory[:] = nodes.req_memory
    nodes.la_alloc_milli_cpu[:] = nodes.alloc_milli_cpu
    nodes.la_alloc_memory[:] = nodes.alloc_memory
    pods = PodTable(p)
    for j in range(p):
        cc, cm = NUMA_TOTALS[j % len(NUMA_TOTALS)], NUMA_TOTALS[(j // 2) % len(NUMA_TOTALS)]
        pods.req_milli_cpu[j] = pods.nonzero_milli_cpu[j] = (cc // 100, -(-cc // 100), 1)[j % 3]
        pods.req_memory[j] = pods.nonzero_memory[j] = (cm // 100, -(-cm // 100), 1)[(j // 3) % 3]
        pods.la_dflt_cpu[j], pods.la_dflt_memory[j] = 250, 200 << 20
    return nodes, nn, pods


def numa_policy_profile(strategy: str = "LeastAllocated") -> SchedulerProfile:
    return SchedulerProfile(fit=NodeResourcesFitArgs(resources={CPU: 1, MEMORY: 1}),
                            numa=NodeNUMAResourceArgs(strategy=strategy, resources={CPU: 1, MEMORY: 3},
                                                      numa_scoring_strategy=strategy))


# ---------------------------------------------------------------------------------------------------------------------
# the commit plan of the reserve walk's contexts, computed on the host from ks_plan.h (as tests/test_commit_plan.py does)
# ---------------------------------------------------------------------------------------------------------------------

PLAN_PROGRAM = r"""
#include <cstdio>
#include "ks_plan.h"
using namespace ks;
int main() {
  int quota, q, cfq, keys, general;
  while (std::scanf("%d %d %d %d %d", &quota, &q, &cfq, &keys, &general) == 5) {
    CommitPlanIn in{};
    in.kc.quota_enable = quota; in.kc.monotone = 1; in.kc.fit_most = 0;
    in.k_cfg = 32; in.nchunks = 1; in.nsc = 2; in.numa_w = kNumaDev; in.q = q;
    in.commit_fq = cfq; in.fq_keys = keys; in.general_mode = general; in.pre_rsv = true;
    const CommitPlan p = commit_plan(in);
    std::printf("%d %d %d %zu %zu\n", (int)p.mono, (int)p.fq, (int)p.fq_keys, p.smem, p.fq_smem);
  }
}
"""
# name: (quota, quota rows, KS_COMMIT_FQ, KS_FQ_KEYS, KS_COMMIT_GENERAL) of run_reserve_walk's contexts (57 nodes = one
# chunk, 32 candidates, two scalar slots, Fit LeastAllocated + LoadAware: monotone)
PLAN_INPUTS = {"mono": (0, 0, 1, 1, 0), "fq-keys": (1, 3, 1, 1, 0), "fq-wave0": (1, 3, 1, 0, 0),
               "general-quota": (1, 3, 0, 1, 0), "general-noquota": (0, 0, 1, 1, 1), "mono-quota": (1, 3, 1, 1, 2)}
_plans = None


def commit_plans() -> dict:
    """{name: {mono, fq, fq_keys, smem, fq_smem}}: which commit kernel ks_plan.h commit_plan selects for each context"""
    global _plans
    if _plans is None:
        import os
        import shutil
        import subprocess
        import tempfile

        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            src, exe = os.path.join(d, "plan.cpp"), os.path.join(d, "plan")
            with open(src, "w") as f:
                f.write(PLAN_PROGRAM)
            subprocess.run([hipcc, "-std=c++17", "-O1", "--cuda-host-only", "-I", os.path.join(root, "koordinator_amd", "csrc"),
                            "-I", os.path.join(root, "include"), "-o", exe, src], check=True)
            text = "".join(" ".join(map(str, v)) + "\n" for v in PLAN_INPUTS.values())
            out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        _plans = {}
        for name, line in zip(PLAN_INPUTS, out):
            m, fq, fk, smem, fsm = map(int, line.split())
            _plans[name] = {"mono": bool(m), "fq": bool(fq), "fq_keys": bool(fk), "smem": smem, "fq_smem": fsm}
    return _plans
