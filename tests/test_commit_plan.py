"""The commit kernel's variant and LDS plan (koordinator_amd/csrc/ks_plan.h commit_plan): a small host program
includes the header, reads the grid of inputs below and prints one plan per row; the output must equal
tests/golden/commit_plan.tsv byte for byte.  The golden file was written by the predicates that commit_plan replaced
(kernel_feat, commit_stat_lds, commit_qcache, commit_rcap, fq_commit, fq_keys, mono_commit, pre_reserve and
commit_attr_set's k loop, copied unchanged into a program of the same shape), every predicate evaluated for every row.
The coverage tests read the golden file alone, so a grid too narrow to reach a decision cannot pass."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "koordinator_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "commit_plan.tsv")

COLS_IN = ("rsv numa dev stat numa_pol held quota_enable monotone fit_most k_cfg nchunks nsc numa_w q "
           "commit_fq fq_keys_env general pre_rsv").split()
COLS_OUT = ("status feat wide k hint_variant stat_lds qcache rcap rsv_bytes dev_bytes numa_bytes smem smem_no_qcache "
            "hint fq fq_keys fq_smem mono mono_smem pre_reserve").split()
LDS = 160 * 1024
QROWS = 128  # kQuotaLdsRows (checked by the program)
BUILT_FEATS = {0, 1, 3, 4, 6, 7, 11, 14, 15, 23, 31}

PROGRAM = r"""
#include <cstdio>
#include "ks_plan.h"
using namespace ks;
static_assert(kQuotaLdsRows == %d && kLdsBytes == %d, "the test's constants");
int main() {
  int v[%d];
  for (;;) {
    for (int& x : v)
      if (std::scanf("%%d", &x) != 1) return 0;
    CommitPlanIn in{};
    in.kc.rsv = v[0]; in.kc.numa = v[1]; in.kc.dev = v[2]; in.kc.stat = v[3]; in.kc.numa_pol = v[4];
    in.dev_held_any = v[5]; in.kc.quota_enable = v[6]; in.kc.monotone = v[7]; in.kc.fit_most = v[8];
    in.k_cfg = v[9]; in.nchunks = v[10]; in.nsc = v[11]; in.numa_w = v[12]; in.q = v[13];
    in.commit_fq = v[14]; in.fq_keys = v[15]; in.general_mode = v[16]; in.pre_rsv = v[17];
    const CommitPlan p = commit_plan(in);
    for (int x : v) std::printf("%%d\t", x);
    std::printf("%%d\t%%d\t%%d\t%%d\t%%d\t%%d\t%%d\t%%d\t%%zu\t%%zu\t%%zu\t%%zu\t%%zu\t%%d\t%%d\t%%d\t%%zu\t%%d\t%%zu\t%%d\n",
                (int)p.status, p.feat, (int)p.wide, (int)p.k, (int)p.hint_variant, (int)p.stat_lds, (int)p.qcache,
                (int)p.rcap, p.rsv_bytes, p.dev_bytes, p.numa_bytes, p.smem, p.smem_no_qcache, (int)p.hint, (int)p.fq,
                (int)p.fq_keys, p.fq_smem, (int)p.mono, p.mono_smem, (int)p.pre_reserve);
  }
}
""" % (QROWS, LDS, len(COLS_IN))

# plugin sets: (rsv, numa, dev, stat, numa_pol, held), by the variant each selects (s: with the dictionary plugins)
PLUG = {
    "f0": (0, 0, 0, 0, 0, 0), "f1": (1, 0, 0, 0, 0, 0), "f3": (1, 1, 0, 0, 0, 0), "f3n": (0, 1, 0, 0, 0, 0),
    "f4": (0, 0, 1, 0, 0, 0), "f4s": (0, 0, 0, 1, 0, 0), "f4ds": (0, 0, 1, 1, 0, 0), "f6": (0, 1, 1, 0, 0, 0),
    "f7": (1, 1, 1, 0, 0, 0), "f7s": (1, 0, 1, 1, 0, 0), "f11": (1, 1, 0, 0, 1, 0), "f11n": (0, 1, 0, 0, 1, 0),
    "f14": (0, 1, 1, 0, 1, 0), "f14s": (0, 1, 1, 1, 1, 0), "f15": (1, 1, 1, 0, 1, 0), "f15s": (1, 1, 1, 1, 1, 0),
    "f23": (1, 0, 1, 0, 0, 1), "f23n": (1, 1, 1, 0, 0, 1), "f31": (1, 1, 1, 0, 1, 1), "f31s": (1, 1, 1, 1, 1, 1),
}


def row(plug, quota=1, mono=1, most=0, k=32, nch=79, nsc=2, w=4, q=16, cfq=1, keys=1, general=0, pre=1):
    return PLUG[plug] + (quota, mono, most, k, nch, nsc, w, q, cfq, keys, general, pre)


def grid():
    """A few small crosses instead of one large one; nchunks runs from 1 to past every variant's refusal point."""
    g = []
    # every plugin set, narrow and wide, small / C5-sized / refused
    g += [row(p, nch=n, w=w) for p in PLUG for w in (4, 8) for n in (1, 1563, 20000) if w == 4 or PLUG[p][4]]
    # candidates x scalar slots x size
    g += [row(p, k=k, nsc=s, nch=n, q=QROWS) for p in ("f0", "f1", "f7", "f15", "f4s")
          for k in (8, 32, 64) for s in (0, 2, 4) for n in (400, 3000)]
    # quota rows around the limits of the LDS cache
    g += [row(p, quota=e, k=k, q=q) for p in ("f0", "f1", "f7") for e in (0, 1) for k in (8, 32)
          for q in (0, 1, QROWS, QROWS + 1)]
    # NUMA width 8: the k shrink (also without policy plugins compiled in: the loop only looks at the width)
    g += [row(p, k=k, nch=n, w=8) for p in ("f11", "f14", "f14s", "f15", "f15s", "f31", "f4s")
          for k in (8, 32, 64) for n in (1, 79, 800, 5000)]
    # the dedicated fq kernel, its slot-key table and the mono kernel: profile x KS_COMMIT_GENERAL x candidates ...
    g += [row("f0", quota=e, mono=m, most=t, general=gm, k=k) for (e, m, t) in ((1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1))
          for gm in (0, 1, 2) for k in (32, 64)]
    # ... x KS_COMMIT_FQ x KS_FQ_KEYS, and the mono image past the LDS
    g += [row("f0", cfq=c, keys=y, k=k) for c in (0, 1) for y in (0, 1) for k in (32, 64)]
    g += [row("f0", quota=0, k=64, nch=n) for n in (3000, 6000)]
    # KS_PRE_RSV
    g += [row(p, pre=e) for p in ("f7", "f11", "f15") for e in (0, 1)]
    # reservation slots from 8 down to 0; at 400 chunks the quota rows fit until the slots (nsc = 4) evict them
    g += [row("f1", k=8, nsc=s, nch=n, q=QROWS) for s in (0, 4) for n in (1, 400, 1563, 3000, 8000, 10000)]
    return list(dict.fromkeys(g))


def golden_lines():
    with open(GOLDEN) as f:
        return f.read().splitlines()


@pytest.fixture(scope="module")
def golden():
    lines = golden_lines()
    assert lines[0].split("\t") == COLS_IN + COLS_OUT
    return [dict(zip(COLS_IN + COLS_OUT, map(int, ln.split("\t")))) for ln in lines[1:]]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    d = tmp_path_factory.mktemp("plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run([hipcc, "-std=c++17", "-O1", "--cuda-host-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), str(src)], check=True)
    text = "".join(" ".join(map(str, r)) + "\n" for r in grid())
    return subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()


def test_golden_is_the_grid(golden):
    assert [tuple(r[c] for c in COLS_IN) for r in golden] == grid()
    assert 100 <= len(golden) <= 500


def test_plans_match_golden(plans):
    want = golden_lines()[1:]
    assert len(plans) == len(want)
    for i, (g, w) in enumerate(zip(plans, want)):
        assert g == w, f"row {i}: " + " ".join(f"{c}={a}->{b}" for c, a, b in
                                                zip(COLS_IN + COLS_OUT, w.split("\t"), g.split("\t")) if a != b or c in COLS_IN)


def twins(golden, differ):
    """pairs of rows whose inputs differ in the column `differ` only"""
    key = [c for c in COLS_IN if c != differ]
    by = {}
    for r in golden:
        by.setdefault(tuple(r[c] for c in key), []).append(r)
    return [(a, b) for rs in by.values() for a, b in itertools.permutations(rs, 2)]


def test_golden_covers_every_decision(golden):
    ok = [r for r in golden if r["status"] == 0]
    assert {r["status"] for r in golden} == {0, 1, 2}, "both refusals"
    assert {r["feat"] for r in ok} == BUILT_FEATS
    assert {r["feat"] for r in ok if r["held"]} == {23, 31}
    for c in ("stat_lds", "qcache", "hint", "fq", "fq_keys", "mono", "pre_reserve"):
        assert {r[c] for r in ok} == {0, 1}, c
    rcaps = {r["rcap"] for r in ok}
    assert {0, 8} <= rcaps and any(0 < v < 8 for v in rcaps)
    for c, vals in (("k_cfg", {8, 32, 64}), ("nsc", {0, 2, 4}), ("numa_w", {4, 8}), ("general", {0, 1, 2}),
                    ("commit_fq", {0, 1}), ("fq_keys_env", {0, 1}), ("pre_rsv", {0, 1}), ("q", {0, 1, QROWS, QROWS + 1})):
        assert {r[c] for r in golden} >= vals, c
    assert min(r["nchunks"] for r in golden) == 1
    for p in {tuple(r[c] for c in COLS_IN[:6]) for r in golden}:
        assert any(r["status"] == 2 for r in golden if tuple(r[c] for c in COLS_IN[:6]) == p), f"{p} never refused"
    assert any(r["wide"] and r["k"] < r["k_cfg"] for r in ok), "the wide k shrink"
    # the mono kernel refused for its own image (always together with the general kernel's: it is the smaller one)
    assert any(not r["mono"] and r["mono_smem"] > LDS for r in golden)
    assert any(r["mono"] for r in ok) and any(r["mono"] and r["quota_enable"] for r in ok)
    # The quota rows evicted by reservation slots: the test that first admits the quota rows reads neither nsc nor
    # rcap, so a twin with another nsc that kept them shows that they first fit here too.
    assert any(a["rsv"] and a["status"] == 0 and not a["qcache"] and b["qcache"] and b["status"] == 0
               for a, b in twins(golden, "nsc")), "quota rows evicted for reservation slots"
    # the slot-key table at 32 candidates and not at 64
    assert any(a["k_cfg"] == 32 and a["fq_keys"] and b["k_cfg"] == 64 and b["fq"] and not b["fq_keys"]
               for a, b in twins(golden, "k_cfg"))
    # the A/B switches each decide something
    assert any(a["fq"] != b["fq"] for a, b in twins(golden, "commit_fq"))
    assert any(a["fq_keys"] != b["fq_keys"] for a, b in twins(golden, "fq_keys_env"))
    assert any(a["mono"] != b["mono"] for a, b in twins(golden, "general"))
    assert any(a["pre_reserve"] != b["pre_reserve"] for a, b in twins(golden, "pre_rsv"))
    # the single-pod commit's image differs only where there are quota rows to drop
    assert all(r["smem_no_qcache"] == r["smem"] for r in golden if not r["qcache"])
    assert any(r["smem_no_qcache"] < r["smem"] for r in ok)
