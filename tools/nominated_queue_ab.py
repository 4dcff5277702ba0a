#!/usr/bin/env python3
"""What the batched queue costs with a nominated table loaded, and what it buys over the per-pod loop, in one process
on C2 at 10,000 pods x 5,000 nodes (synth.c2):

  a  ks_schedule, no table                                  (run it on the parent commit too: --only a)
  b  ks_schedule_nominated, empty table
  c  ks_schedule_nominated, 50 and 200 rows, 20 owner pods
  d  the per-pod loop a shim runs without it for the 200-row case: eval_pod_summary_nominated -> assume ->
     delete_nominated (one round trip per pod)

The pods are staged once per variant; a round restores the checkpoint (state and table) and times ks_schedule_staged
with the host clock (the call ends in a stream synchronize).  Warm-up rounds first, then rounds that take the variants
in turn so that they are measured next to each other; the figure is the median over the rounds with their min and max
as the spread.  Needs the GPU; there is no fallback.

usage: python tools/nominated_queue_ab.py [--out FILE] [--rounds 9] [--warmup 3] [--loop-rounds 2] [--only a]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from koordinator_amd import runtime, synth  # noqa: E402
from koordinator_amd.cluster import NominatedTable  # noqa: E402

N_NODES, N_PODS, OWNERS = 5000, 10_000, 20


def table(w, rows, rng):
    """`rows` rows of priority 1000 on rows / 2 random nodes, each a quarter of its node's free cpu; the first OWNERS
    rows belong to pods of the queue"""
    nodes = rng.choice(w.nodes.n, max(rows // 2, 1), replace=False)
    t = NominatedTable(rows)
    for r in range(rows):
        i = int(nodes[r % len(nodes)])
        t.node[r], t.priority[r], t.id[r] = i, 1000, r
        t.req[0, r] = max(int(w.nodes.alloc_milli_cpu[i] - w.nodes.req_milli_cpu[i]) // 4, 0)
        t.req[1, r] = 1 << 28
    return t


def nominations(w, t, rng):
    p = w.pods.n
    prio = rng.choice((500, 1000, 1500), p).astype(np.int64)
    nn = np.full(p, -1, np.int64)
    sid = np.full(p, -1, np.int64)
    if t is not None:
        for k, pos in enumerate(np.linspace(0, p - 1, OWNERS).astype(int)):
            prio[pos], nn[pos], sid[pos] = 1000, t.node[k], t.id[k]
    return prio, nn, sid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-rounds", type=int, default=2)
    ap.add_argument("--only", choices=["a"])
    a = ap.parse_args()
    runtime.lib()
    rng = np.random.default_rng(3)
    w = synth.c2(n_nodes=N_NODES, n_pods=N_PODS)
    variants = [("a schedule, no table", None, False)]
    if not a.only:
        variants += [("b schedule_nominated, empty table", None, True),
                     ("c schedule_nominated, 50 rows", table(w, 50, rng), True),
                     ("c schedule_nominated, 200 rows", table(w, 200, rng), True)]
    evs, info = [], {}
    try:
        for name, t, nominated in variants:
            ev = runtime.Evaluator(w.cfg, w.nodes.copy(), **w.tables())
            evs.append(ev)
            if t is not None:
                ev.load_nominated(t)
            ev.checkpoint()
            if nominated:
                ev.stage_nominated(w.pods, *nominations(w, t, rng))
            else:
                ev.stage(w.pods)
        times = {name: [] for name, _, _ in variants}
        for rnd in range(a.warmup + a.rounds):
            for (name, _, _), ev in zip(variants, evs):
                ev.restore()
                t0 = time.perf_counter()
                ev.schedule_staged()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd >= a.warmup:
                    times[name].append(dt)
                st = ev.stats()
                info[name] = (st["passes"], st["cut_passes"], st["diag"][4], st["diag"][5], int((ev.fetch()["status"] == 0).sum()))
        loop = []
        if not a.only:
            name, t, _ = variants[-1]
            ev = evs[-1]
            prio, nn, sid = nominations(w, t, np.random.default_rng(3))
            pods = [w.pods.rows([i]) for i in range(N_PODS)]
            for _ in range(a.loop_rounds):
                ev.restore()
                t0 = time.perf_counter()
                for i in range(N_PODS):
                    s = ev.eval_pod_summary_nominated(pods[i], int(prio[i]), int(nn[i]), int(sid[i]), top_n=1)
                    if s["best_node"] >= 0:
                        ev.assume(pods[i], s["best_node"])
                        if sid[i] >= 0:
                            ev.delete_nominated([int(sid[i])])
                loop.append((time.perf_counter() - t0) * 1e3)
    finally:
        for ev in evs:
            ev.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# C2, {N_PODS} pods x {N_NODES} nodes, {OWNERS} owner pods: ms per ks_schedule_staged, median over {a.rounds} "
             f"interleaved rounds [min .. max], warm-up {a.warmup} rounds; us per pod",
             "# variant | ms | us per pod | passes | cut passes | owner passes | rows retired | pods placed"]
    for name, _, _ in variants:
        v = times[name]
        lines.append(f"{name} | {med[name]:.2f} [{min(v):.2f} .. {max(v):.2f}] | {med[name] * 1e3 / N_PODS:.2f} | "
                     + " | ".join(str(x) for x in info[name]))
    if loop:
        ml = statistics.median(loop)
        lines.append(f"d per-pod loop, 200 rows (host clock, {a.loop_rounds} rounds) | {ml:.1f} [{min(loop):.1f} .. {max(loop):.1f}] | "
                     f"{ml * 1e3 / N_PODS:.1f} | - | - | - | - | -")
        base = med[variants[0][0]]
        for name, _, _ in variants[1:]:
            lines.append(f"# ({name}) / (a) = {med[name] / base:.2f}")
        lines.append(f"# (d) / (c, 200 rows) = {ml / med[variants[-1][0]]:.1f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
