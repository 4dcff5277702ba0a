"""Host side of ks_eval_pod_summary (no GPU): the ctypes mirror of ks_pod_summary against the built library's layout
word, the export, the FitError text from the reason histogram, and the --debug-scores table rendered from a summary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from koordinator_amd import abi, debug_scores
from koordinator_amd.config import SchedulerProfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "koordinator_amd", "libkoordgpu.so")


def test_struct_mirror():
    assert abi.KS_SUMMARY_MAX_TOP == 64
    assert C.sizeof(abi.KsPodSummary) == 8 * 3 + 8 * 32 + 8 + 4 + 4
    assert abi.KsPodSummary.reason_nodes.offset == 24 and abi.KsPodSummary.best_total.offset == 280
    assert abi.KsPodSummary.best_node.offset == 288 and abi.KsPodSummary.top_count.offset == 292
    with open(os.path.join(ROOT, "include", "koordgpu.h")) as f:
        header = f.read()
    assert f"#define KS_SUMMARY_MAX_TOP {abi.KS_SUMMARY_MAX_TOP}\n" in header
    assert f"#define KS_ABI_VERSION {abi.KS_ABI_VERSION}\n" in header


def test_library_reports_the_struct_size():
    if not os.path.exists(LIB):
        pytest.skip("libkoordgpu.so not built (run __graft_entry__.build())")
    from koordinator_amd import runtime

    L = runtime.lib()
    got = (C.c_int64 * abi.KS_ABI_LAYOUT_WORDS)()
    assert L.ks_abi_layout(got, abi.KS_ABI_LAYOUT_WORDS) == abi.KS_ABI_LAYOUT_WORDS == 18
    assert got[17] == C.sizeof(abi.KsPodSummary) == runtime.expected_layout()[17]
    assert got[0] == abi.KS_ABI_VERSION == 11


def test_symbol_listed_and_exported():
    assert "ks_eval_pod_summary" in abi.EXPORTED_SYMBOLS
    if not os.path.exists(LIB):
        pytest.skip("libkoordgpu.so not built (run __graft_entry__.build())")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    assert any(line.split()[-1] == "ks_eval_pod_summary" and " T " in line for line in nm.splitlines())


def test_fit_error_message():
    hist = np.zeros(32, np.int64)
    hist[abi.KS_R_FIT_CPU.bit_length() - 1] = 3000
    hist[abi.KS_R_TAINT.bit_length() - 1] = 2000
    hist[abi.KS_R_FIT_MEMORY.bit_length() - 1] = 41
    hist[31] = 7
    # "<count> <reason>" strings sorted as strings: "2000 ..." < "3000 ..." < "41 ..." < "7 ..."
    assert debug_scores.fit_error_message(5000, hist) == (
        "0/5000 nodes are available: 2000 node(s) had untolerated taint, 3000 Insufficient cpu, "
        "41 Insufficient memory, 7 node(s) didn't satisfy existing pods anti-affinity rules.")
    assert debug_scores.fit_error_message(0, np.zeros(32, np.int64)) == "0/0 nodes are available."
    assert len(debug_scores.REASON_TEXT) == 32 and len(set(debug_scores.REASON_TEXT)) == 32


class StubEvaluator:
    """eval_pod_summary from a canned dict; eval_pod must not be reached for top_n <= KS_SUMMARY_MAX_TOP"""

    def __init__(self, summary):
        self.summary = summary
        self.calls = []

    def eval_pod_summary(self, pod, top_n=0, unresolvable_mask=0, want_bits=False):
        self.calls.append(top_n)
        s = dict(self.summary)
        for k in ("top_nodes", "top_totals", "top_scores"):
            s[k] = s[k][:top_n]
        return s

    def eval_pod(self, pod):
        raise AssertionError("the whole matrix was asked for")


def canned(feasible):
    scores = np.zeros((3, abi.KS_NUM_SCORE_PLUGINS), np.int64)
    scores[:, abi.KS_SCORE_FIT] = [90, 80, 80]
    scores[:, abi.KS_SCORE_LOADAWARE] = [50, 60, 60]
    return {"nodes": 9, "feasible": feasible, "unresolvable": 0, "reason_nodes": np.zeros(32, np.int64),
            "best_node": 7, "best_total": 140, "top_nodes": np.array([7, 2, 4], np.int32),
            "top_totals": np.array([140, 140, 140], np.int64), "top_scores": scores}


def test_debug_table_from_a_canned_summary():
    cfg = SchedulerProfile().to_ks_config()
    assert cfg.fit.enable_score and cfg.loadaware.enable_score
    assert cfg.fit.plugin_weight == 1 and cfg.loadaware.plugin_weight == 1
    names = [f"node-{i}" for i in range(9)]
    ev = StubEvaluator(canned(5))
    got = debug_scores.eval_debug_table_top(ev, cfg, None, names, 2, "default/p")
    cols = [n for n, _, enabled, _ in sorted(debug_scores.SCORE_PLUGINS, key=lambda p: p[0]) if enabled(cfg)]
    zeros = {n: 0 for n in cols}

    def line(rank, node, total, **by_plugin):
        cells = dict(zeros, **by_plugin)
        return "| " + " | ".join(str(c) for c in [rank, "default/p", node, total] + [cells[n] for n in cols]) + " |"

    assert got.split("\n") == [
        "| # | Pod | Node | Score | " + " | ".join(cols) + " |",
        "|" + "|".join([" --- "] * 3 + [" ---:"] * (1 + len(cols))) + "|",
        line(0, "node-7", 140, NodeResourcesFit=90, LoadAwareScheduling=50),
        line(1, "node-2", 140, NodeResourcesFit=80, LoadAwareScheduling=60),
    ]
    assert ev.calls == [2]
    # nothing is logged for top_n <= 0 or fewer than two feasible nodes
    assert debug_scores.eval_debug_table_top(ev, cfg, None, names, 0, "default/p") is None
    assert debug_scores.eval_debug_table_top(StubEvaluator(canned(1)), cfg, None, names, 5, "default/p") is None
    # more rows than the device keeps: the whole-matrix path serves them
    with pytest.raises(AssertionError, match="whole matrix"):
        debug_scores.eval_debug_table_top(ev, cfg, None, names, abi.KS_SUMMARY_MAX_TOP + 1, "default/p")
