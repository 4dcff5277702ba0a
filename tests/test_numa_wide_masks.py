"""The IterateBitMasks order table of the 8-wide NUMA policy path (koordinator_amd/csrc/ks_numa_masks.h): a tiny host
program includes the header and prints the table; it must list, for K = 1..8, the masks by size 1..K, each size in
lexicographic order of its id list (bitmask.go:206-222), and for K <= 4 agree with the 64-bit constants the 4-wide
path reads its order from (ks_numa.h numa_mask_table)."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "koordinator_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "ks_numa_masks.h"
int main() {
  constexpr ks::NumaMaskOrder t = ks::make_numa_mask_order();
  for (int K = 0; K <= ks::kNumaMaskMaxK; ++K) {
    std::printf("%d:", K);
    for (int i = 0; i < ks::kNumaMaskRow; ++i) std::printf(" %u", (unsigned)t.m[K][i]);
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("masks")
    src, exe = d / "masks.cpp", d / "masks"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        k, vals = line.split(":")
        rows[int(k)] = [int(v) for v in vals.split()]
    return rows


def iterate_bit_masks(K):
    return [sum(1 << i for i in ids) for size in range(1, K + 1) for ids in itertools.combinations(range(K), size)]


def test_table_shape(table):
    assert sorted(table) == list(range(9))
    assert all(len(r) == 255 for r in table.values())
    assert table[0] == [0] * 255


@pytest.mark.parametrize("K", range(1, 9))
def test_order_is_iterate_bit_masks(table, K):
    want = iterate_bit_masks(K)
    assert len(want) == (1 << K) - 1
    assert table[K][: len(want)] == want
    assert table[K][len(want):] == [0] * (255 - len(want))


def test_narrow_constants_agree(table):
    """numa_mask_table's constants: mask i in bits [4i, 4i + 4)"""
    text = open(os.path.join(CSRC, "ks_numa.h")).read()
    m = re.search(r"numa_mask_table\(int K\) \{\s*return K <= 1 \? (0x[0-9A-Fa-f]+)ull : \(K == 2 \? (0x[0-9A-Fa-f]+)ull : "
                  r"\(K == 3 \? (0x[0-9A-Fa-f]+)ull : (0x[0-9A-Fa-f]+)ull\)\);", text)
    assert m, "numa_mask_table not found in ks_numa.h"
    for K, lit in zip(range(1, 5), m.groups()):
        v = int(lit, 16)
        nib = [(v >> (4 * i)) & 0xF for i in range((1 << K) - 1)]
        assert nib == table[K][: len(nib)], f"K={K}"
        assert v >> (4 * len(nib)) == 0
