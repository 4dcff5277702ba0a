"""The C oracle's eval_pod against the Go formulas restated in Python integers (score_edge_util.py), on the boundary
case set: quotients 100 (h - p) / c that are integers or one unit (1/c) off one, capacities around 2^43 and up to
2^56 - 1, primes, zero capacities, pod requests around 2^46.  Every comparison is exact.  With this the oracle is a
checked middleman: tests/test_gpu_score_edges.py compares the device with it (and with the Python reference) on the
same cases."""
from fractions import Fraction

import numpy as np
import pytest

import score_edge_util as U
from koordinator_amd import abi


@pytest.fixture(scope="module")
def cases():
    return [U.Case(s) for s in U.matrix()]


def test_case_set_conditions(cases):
    tri = U.all_triples()
    on_integer = [t for t in tri if (100 * t[1]) % t[0] == 0]
    one_below = [t for t in tri if (100 * t[1]) % t[0] >= t[0] - 100]
    assert len(on_integer) >= 100 and len(one_below) >= 100, (len(on_integer), len(one_below))
    down, up = U.reciprocal_directions()
    assert down and up, "fl(1/c) must round in both directions among the capacities below 2^43"
    for c in down:
        assert Fraction(1.0 / c) < Fraction(1, c)
    for c in up:
        assert Fraction(1.0 / c) > Fraction(1, c)
    assert all(U.is_prime(p) for p in U.PRIMES) and sorted(len(str(p)) for p in U.PRIMES) == [5, 5, 11, 11, 13, 13]
    assert {1, 2, 3, 7, 100, 101, 999, 3 << 37, 2 ** 43 - 3, 2 ** 43 - 1, 2 ** 43, 2 ** 43 + 1, 2 ** 47 + 12345,
            2 ** 55 + 7, 2 ** 56 - 1} <= set(U.CAPS)
    assert {0, 1, 12345, 2 ** 46 - 1, 2 ** 46, 2 ** 46 + 1, 2 ** 55} == set(U.POD_REQUESTS)
    # what the evaluation cases really carry on their terms: the same two counts, every capacity, overcommitted and
    # zero-capacity terms, and the node layout
    used = [t for c in cases for row in c.used for t in row]
    real = set(t for t in used if t is not None)
    assert sum((100 * d) % c == 0 for c, d, _ in real) >= 100
    assert sum((100 * d) % c >= c - 100 for c, d, _ in real) >= 100
    assert {c for c, _, _ in real} == set(U.CAPS)
    assert any(d < 0 for _, d, _ in real) and any(t is None for t in used)
    assert {p for _, _, p in real} >= set(U.POD_REQUESTS)
    for c in cases:
        assert c.nodes.n <= 512 and c.nodes.n % 64 != 0
    # the layout as the built tables hold it: a node counts as big when one of its score-term capacities is >= 2^43
    # (what prep_nodes_kernel flags); a node dealt as small never is, and every case keeps a chunk of each kind
    for c in cases:
        big = c.big_nodes()
        dealt = np.array([U.node_is_big(i) for i in range(c.nodes.n)])
        assert not (big & ~dealt & ~c.turned_big).any(), f"{c.spec.name()}: a small node holds a capacity >= 2^43"
        assert (big | ~dealt).all(), f"{c.spec.name()}: node {int(np.nonzero(dealt & ~big)[0][0])} dealt as big holds none"
        chunks = [big[k:k + 64] for k in range(0, c.nodes.n, 64)]
        assert any(ch.all() for ch in chunks), c.spec.name()
        if not c.turned_big.any():  # (a big request on a Filter-checked term leaves no small node: every lane int64)
            assert any(not ch.any() for ch in chunks), c.spec.name()
            alt = [ch for ch in chunks if len(ch) == 64 and ch.any() and not ch.all()]
            assert any((ch[0::2] != ch[1::2]).all() for ch in alt), f"{c.spec.name()}: no chunk alternates lane by lane"
    assert sum(not c.turned_big.any() for c in cases) > len(cases) * 3 // 4


def test_case_set_tells_where_the_f64_path_must_end():
    """Replayed in exact arithmetic (score_edge_util.least_f64 / most_f64), the device's f64 formula holds on every
    headroom of the capacities below 2^43 and is off by one at 2^44 - 15 and 2^44 - 17: the device test fails if the switch to int64
    (kBigCap) moves up to 2^44.  (A pod-side switch, kBigReq, moved from 2^46 to 2^47 cannot show: such a request is
    larger than every capacity below 2^43, so the term is 0 or 100 whatever the rounding, and 100 p < 2^54 is a
    multiple of 4, hence still exact in f64.)"""
    def wrong(c):
        return [(d, p) for d in U.headrooms(c) for p in (0, 1, 12345) if d + p <= c and
                (U.least_f64(c, d + p, p) != U.least(c - d, c) or U.most_f64(c, d + p, p) != U.most(c - d, c))]

    for c in U.CAPS:
        if c < U.BIG_CAP:
            assert not wrong(c), c
    assert wrong((1 << 44) - 15) and wrong((1 << 44) - 17)
    for p in (U.BIG_REQ, (1 << 47) - 1):
        assert p > U.BIG_CAP and 100 * p < 2 ** 54 and (100 * p) % 4 == 0 and int(float(100 * p)) == 100 * p


def test_matrix_covers_the_issue(cases):
    sp = [c.spec for c in cases]
    assert {s.strategy for s in sp} == {"LeastAllocated", "MostAllocated"}
    assert {s.fit_w for s in sp} == {(1, 1), (1, 100), (100, 1), (3, 7)} and any(s.eph_w for s in sp)
    assert {(s.nsc, s.pod_scalars) for s in sp} >= {(n, r) for n in (0, 2, 4) for r in (False, True)}
    assert {s.la_w for s in sp} == {(1, 1), (100, 1)} and {s.la_mode for s in sp} == {"dflt", "lim", "req"}
    assert {(s.prod_usage, s.prod_pod) for s in sp} == {(a, b) for a in (False, True) for b in (False, True)}
    assert (85, 70) in {s.sf for s in sp}
    assert {s.numa for s in sp} == {None, 1.0, 1.5, 1.0000001, 1.25} and {s.bind for s in sp} == {False, True}
    assert float(24000 * 1.5).is_integer() and U.amplify(7000, 1.0000001) == 7001


def test_oracle_matches_the_python_reference(oracle_lib, cases):
    for c in cases:
        orc = oracle_lib.Oracle(c.cfg, c.nodes.copy(), **c.tables())
        try:
            reasons, scores, total = orc.eval_pod(c.pod)
        finally:
            orc.close()
        tag = c.spec.name()
        assert not reasons.any(), f"{tag}: node {int(np.nonzero(reasons)[0][0])} infeasible ({int(reasons[reasons != 0][0]):#x})"
        for col, key in ((abi.KS_SCORE_FIT, "fit"), (abi.KS_SCORE_LOADAWARE, "la"), (abi.KS_SCORE_NUMA, "numa")):
            bad = np.nonzero(scores[:, col] != c.want[key])[0]
            assert not len(bad), f"{tag}: {key} differs on {len(bad)} nodes; node {int(bad[0])}: oracle " \
                                 f"{int(scores[bad[0], col])}, reference {int(c.want[key][bad[0]])}, terms {c.used[bad[0]]}"
        assert np.array_equal(total, c.want["total"]), f"{tag}: total"
