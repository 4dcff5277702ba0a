#!/usr/bin/env python3
"""A/B of the per-pod evaluation's two ways back to the host, in one process on one context and one pod:

  A  Evaluator.eval_pod            reasons [n], scores [n, KS_NUM_SCORE_PLUGINS] and totals [n] copied to the host
  B  Evaluator.eval_pod_summary    top_n=16, want_bits=True: the summary, 16 rows and the two bitmasks

at C2's 5,000 nodes and at 100,000 nodes (synth.c2).  Each call ends in a stream synchronize, so the host clock around
a call is the call's time.  Per size: a warm-up of both, then rounds that alternate A and B (other work shares the
host, so the two are measured next to each other); the figure is the median over rounds of a round's mean call time,
with the rounds' min and max as the spread.  Before timing, B is checked against the numpy reduction of A's arrays at
that size.  Needs the GPU; there is no fallback.

usage: python tools/eval_summary_ab.py [--out FILE] [--rounds 15] [--calls 40] [--warmup 30]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from koordinator_amd import abi, runtime, synth  # noqa: E402

TOP_N = 16
MASK = abi.KS_R_FIT_CPU | abi.KS_R_FIT_MEMORY


def same_answer(ev, pod):
    r, s, t = ev.eval_pod(pod)
    got = ev.eval_pod_summary(pod, top_n=TOP_N, unresolvable_mask=MASK, want_bits=True)
    idx = np.flatnonzero(r == 0)
    top = idx[np.lexsort((idx, -t[idx]))][:TOP_N]
    n = len(r)
    bits = np.unpackbits(got["feasible_bits"].view(np.uint8), bitorder="little")
    ubits = np.unpackbits(got["unresolvable_bits"].view(np.uint8), bitorder="little")
    return (got["feasible"] == len(idx) and np.array_equal(got["top_nodes"], top)
            and np.array_equal(got["top_totals"], t[top]) and np.array_equal(got["top_scores"], s[top])
            and np.array_equal(bits[:n].astype(bool), r == 0) and not bits[n:].any()
            and np.array_equal(ubits[:n].astype(bool), (r & np.uint32(MASK)) != 0)
            and all(got["reason_nodes"][b] == int(((r >> np.uint32(b)) & np.uint32(1)).sum()) for b in range(32)))


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--nodes", type=int, nargs="*", default=[5000, 100_000])
    a = ap.parse_args()
    runtime.lib()
    lines = [f"# eval_pod (A) vs eval_pod_summary top_n={TOP_N} want_bits (B): us per call, median over {a.rounds} "
             f"alternating rounds of {a.calls} calls each [min .. max of the rounds], warm-up {a.warmup} calls each",
             "# nodes | copied to host A (bytes) | copied B (bytes) | A us | B us | A / B | B == reduce(A)"]
    for n in a.nodes:
        w = synth.c2(n_nodes=n, n_pods=64)
        ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
        try:
            pod = w.pods.rows([0])
            fa = lambda: ev.eval_pod(pod)  # noqa: E731
            fb = lambda: ev.eval_pod_summary(pod, top_n=TOP_N, unresolvable_mask=MASK, want_bits=True)  # noqa: E731
            ok = same_answer(ev, pod)
            timed(fa, a.warmup)
            timed(fb, a.warmup)
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(timed(fa, a.calls))
                tb.append(timed(fb, a.calls))
            ma, mb = statistics.median(ta), statistics.median(tb)
            bytes_a = n * (4 + 8 * abi.KS_NUM_SCORE_PLUGINS + 8)
            bytes_b = (8 * 3 + 8 * 32 + 16) + abi.KS_SUMMARY_MAX_TOP * (4 + 8 + 8 * abi.KS_NUM_SCORE_PLUGINS) \
                + 2 * 8 * ((n + 63) // 64)
            lines.append(f"{n} | {bytes_a} | {bytes_b} | {ma:.1f} [{min(ta):.1f} .. {max(ta):.1f}] | "
                         f"{mb:.1f} [{min(tb):.1f} .. {max(tb):.1f}] | {ma / mb:.2f} | {ok}")
        finally:
            ev.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(line.endswith("True") for line in lines[2:]) else 1


if __name__ == "__main__":
    sys.exit(main())
