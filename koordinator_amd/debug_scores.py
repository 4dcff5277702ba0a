"""The --debug-scores top-N table (frameworkext/debug.go:61-108), fed by the device's Score results.

koord-scheduler's framework extender logs this table after RunScorePlugins (framework_extender.go:254-257) when
`--debug-scores` / `-s` is above 0 (debug.go:36-48).  Each row is a feasible node; its cells are the plugins' weighted,
normalized scores, as RunScorePlugins returns them (v1.24 framework: NormalizeScore, then score x weight).  The device
returns the same numbers through `ks_eval_pod` (un-weighted per-plugin scores, which `plugin_scores` multiplies by the
profile's weights), so the host renders the table without re-running any plugin.

Parity: the markdown layout is pinned by the reference's TestDebugScores (debug_test.go:91-176, the golden in
tests/test_debug_scores.py).  Order of equal totals is not pinned: debug.go sorts with Go's unstable sort.Slice; here
equal totals keep node order (a stable sort).
"""
from __future__ import annotations

import numpy as np

from . import abi

# (plugin name, score column of ks_eval_pod, enabled(cfg), weight(cfg))
SCORE_PLUGINS = [
    ("NodeResourcesFit", abi.KS_SCORE_FIT, lambda c: c.fit.enable_score, lambda c: c.fit.plugin_weight),
    ("LoadAwareScheduling", abi.KS_SCORE_LOADAWARE, lambda c: c.loadaware.enable_score,
     lambda c: c.loadaware.plugin_weight),
    ("Reservation", abi.KS_SCORE_RESERVATION, lambda c: c.reservation.enable, lambda c: c.reservation.plugin_weight),
    ("NodeNUMAResource", abi.KS_SCORE_NUMA, lambda c: c.numa.enable, lambda c: c.numa.plugin_weight),
    ("DeviceShare", abi.KS_SCORE_DEVICESHARE, lambda c: c.deviceshare.enable, lambda c: c.deviceshare.plugin_weight),
    ("NodeResourcesBalancedAllocation", abi.KS_SCORE_BALANCED, lambda c: c.balanced.enable,
     lambda c: c.balanced.plugin_weight),
    ("TaintToleration", abi.KS_SCORE_TAINT, lambda c: c.taint.enable_score, lambda c: c.taint.plugin_weight),
    ("NodeAffinity", abi.KS_SCORE_NODE_AFFINITY, lambda c: c.affinity.enable_score, lambda c: c.affinity.plugin_weight),
    ("PodTopologySpread", abi.KS_SCORE_TOPOLOGY_SPREAD, lambda c: c.topology.enable, lambda c: c.topology.spread_weight),
    ("InterPodAffinity", abi.KS_SCORE_POD_AFFINITY, lambda c: c.topology.enable, lambda c: c.topology.affinity_weight),
]


def plugin_scores(cfg, reasons, scores):
    """RunScorePlugins' result over the feasible nodes: (feasible node indices in node order, {plugin: weighted scores
    aligned with them}) from ks_eval_pod's reasons [n] and un-weighted scores [n, KS_NUM_SCORE_PLUGINS]."""
    feas = np.flatnonzero(np.asarray(reasons) == 0)
    scores = np.asarray(scores, np.int64)
    out = {}
    for name, col, enabled, weight in SCORE_PLUGINS:
        if enabled(cfg):
            out[name] = [int(v) * int(weight(cfg)) for v in scores[feas, col]]
    return feas, out


def debug_scores(top_n: int, pod_ref: str, plugin_to_node_scores: dict, node_names) -> str:
    """debugScores (debug.go:61-108) rendered as go-pretty's RenderMarkdown: rows are the first top_n nodes by total
    score (descending), columns `#`, `Pod` (klog.KObj: namespace/name), `Node`, `Score` and the plugins in name order;
    numeric columns right-aligned."""
    names = sorted(plugin_to_node_scores)
    total = [sum(plugin_to_node_scores[p][i] for p in names) for i in range(len(node_names))]
    order = sorted(range(len(node_names)), key=lambda i: -total[i])

    def row(cells):
        return "| " + " | ".join(str(c).replace("|", "\\|") for c in cells) + " |"

    lines = [row(["#", "Pod", "Node", "Score"] + names),
             "|" + "|".join([" --- "] * 3 + [" ---:"] * (1 + len(names))) + "|"]
    for rank, i in enumerate(order[:max(top_n, 0)]):
        lines.append(row([rank, pod_ref, node_names[i], total[i]] + [plugin_to_node_scores[p][i] for p in names]))
    return "\n".join(lines)


def eval_debug_table(ev, cfg, pod, node_names, top_n: int, pod_ref: str):
    """The table the extender logs for pod 0 of `pod` against the evaluator's current state, or None where it logs
    nothing: top_n <= 0 (debug.go hook), or fewer than two feasible nodes (the v1.24 scheduler skips scoring for one
    feasible node and fails the pod for none)."""
    if top_n <= 0:
        return None
    reasons, scores, _ = ev.eval_pod(pod)
    feas, per_plugin = plugin_scores(cfg, reasons, scores)
    if len(feas) < 2:
        return None
    return debug_scores(top_n, pod_ref, per_plugin, [node_names[i] for i in feas])


# FitError text of each reason bit (index b = KS_R_* bit 1 << b), from the comments next to the KS_R_* defines in
# include/koordgpu.h: the quoted status message where the comment quotes one, the reference's error name otherwise.
REASON_TEXT = [
    "Too many pods",
    "Insufficient cpu",
    "Insufficient memory",
    "Insufficient ephemeral-storage",
    "Insufficient <scalar>",
    "ErrReasonUsageExceedThreshold cpu",
    "ErrReasonUsageExceedThreshold memory",
    "ErrReasonAggregatedUsageExceedThreshold",
    "filterProdUsage",
    "ErrReasonReservationAffinity",
    "filterWithReservations: no matched reservation satisfies the pod",
    "ErrInsufficientAmplifiedCPU",
    "ErrInvalidCPUAmplificationRatio",
    "Insufficient gpu devices",
    "node has no (healthy) GPU",
    "ErrInvalidCPUTopology",
    "node(s) NUMA Topology affinity error",
    "Insufficient NUMA <resource>",
    "node(s) missing NUMA resources",
    "Insufficient rdma devices",
    "node(s) Joint-Allocate rules not met",
    "not enough cpus available to satisfy request",
    "ErrInvalidRequestedCPUs",
    "ErrCPUBindPolicyConflict",
    "ErrSMTAlignmentError",
    "node(s) had untolerated taint",
    "node(s) didn't match Pod's node affinity/selector",
    "node(s) didn't have free ports for the requested pod ports",
    "node(s) didn't match pod topology spread constraints",
    "node(s) didn't match pod affinity rules",
    "node(s) didn't match pod anti-affinity rules",
    "node(s) didn't satisfy existing pods anti-affinity rules",
]


def fit_error_message(n_nodes: int, reason_nodes, reason_text=REASON_TEXT) -> str:
    """The scheduler's FitError text for a pod no node fits, "0/N nodes are available: <count> <reason>, ... .", from
    ks_eval_pod_summary's histogram (reason_nodes[b] = nodes whose reasons word has bit b): one "<count> <reason>"
    per non-empty bin, sorted as strings before they are joined, as upstream's FitError.Error does.  A node with two
    reasons counts under both.  KS_R_LA_AGGREGATED and KS_R_LA_PROD qualify the LoadAware bits and are listed like any
    other bin.  Parity unpinned: upstream's framework/types.go is not on disk, so the sentence's exact form (the
    prefix, ", " between reasons, the closing ".") is this project's reading of it, and the texts of the bins whose
    header comment names an error constant instead of quoting a message are those names."""
    parts = sorted(f"{int(c)} {reason_text[b]}" for b, c in enumerate(reason_nodes) if int(c) > 0)
    msg = f"0/{int(n_nodes)} nodes are available"
    return msg + (": " + ", ".join(parts) + "." if parts else ".")


def eval_debug_table_top(ev, cfg, pod, node_names, top_n: int, pod_ref: str):
    """eval_debug_table from the device's own reduction (Evaluator.eval_pod_summary): the top_n rows, already in the
    table's order (total descending, equal totals in node order), are all that leaves the device.  None under the same
    conditions; top_n above KS_SUMMARY_MAX_TOP is served by eval_debug_table."""
    if top_n <= 0:
        return None
    if top_n > abi.KS_SUMMARY_MAX_TOP:
        return eval_debug_table(ev, cfg, pod, node_names, top_n, pod_ref)
    s = ev.eval_pod_summary(pod, top_n=top_n)
    if s["feasible"] < 2:
        return None
    rows = [int(i) for i in s["top_nodes"]]
    _, per_plugin = plugin_scores(cfg, np.zeros(len(rows), np.uint32), s["top_scores"])
    return debug_scores(top_n, pod_ref, per_plugin, [node_names[i] for i in rows])
