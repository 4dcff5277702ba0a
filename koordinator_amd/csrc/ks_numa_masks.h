// ks_numa_masks.h — the IterateBitMasks order (bitmask.go:206-222) for K <= 8 NUMA nodes as a compile-time table.
// No HIP dependency: a host program can include it (tests/test_numa_wide_masks.py prints it).
//
// Row K of the table lists the 2^K - 1 non-empty masks over NUMA ids 0..K-1 by size 1..K, each size in
// lexicographic order of its ascending id list; the rest of the row is 0.
#pragma once

#include <stdint.h>

namespace ks {

constexpr int kNumaMaskMaxK = 8;
constexpr int kNumaMaskRow = 255;  // 2^8 - 1

struct NumaMaskOrder {
  uint8_t m[kNumaMaskMaxK + 1][kNumaMaskRow];
};

constexpr NumaMaskOrder make_numa_mask_order() {
  NumaMaskOrder t{};
  for (int K = 1; K <= kNumaMaskMaxK; ++K) {
    int n = 0;
    for (int size = 1; size <= K; ++size) {
      int idx[kNumaMaskMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < size; ++i) idx[i] = i;
      for (;;) {
        uint32_t mask = 0;
        for (int i = 0; i < size; ++i) mask |= 1u << idx[i];
        t.m[K][n++] = (uint8_t)mask;
        int i = size - 1;
        while (i >= 0 && idx[i] == K - size + i) --i;
        if (i < 0) break;
        ++idx[i];
        for (int k = i + 1; k < size; ++k) idx[k] = idx[k - 1] + 1;
      }
    }
  }
  return t;
}

}  // namespace ks
