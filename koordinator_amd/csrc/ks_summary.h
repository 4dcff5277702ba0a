// ks_summary.h — ks_eval_pod_summary's reductions of one pod's evaluation.
//
// ks_eval_pod's kernels leave reasons [n], the per-plugin scores [n][KS_NUM_SCORE_PLUGINS] and totals [n] in the
// context's evaluation buffer.  A shim that owns the cycle needs four small things of them: the feasible set, selectHost's
// winner (lowest index among equal totals), the per-reason node counts of the FitError message, and the first rows of
// the --debug-scores table.  Two kernels on the evaluation's stream produce them, so only those leave the device:
//
//   summary_block_kernel  256 nodes per workgroup, one wave per 64-node word of the two bitmasks (ballots; lanes at or
//                         past n hold reasons 0 / not feasible, so they reach no ballot, bin or sort key).  The 32
//                         reason bits are a ballot + popcount each into LDS bins, written as the workgroup's own row
//                         (no global atomics, nothing to clear between calls).  Each feasible node ranks its (total,
//                         node) pair among the workgroup's by counting the pairs that beat it -- every lane reads the
//                         same LDS word, a broadcast, so no bank conflicts and no barriers inside the loop -- and the
//                         first k = max(top_n, 1) ranks go to the workgroup's partial list, padded with a sentinel that
//                         sorts last.  With `only` >= 0 and that node feasible, it alone counts as feasible.
//   summary_merge_kernel  one workgroup of 16 waves.  A wave holds a sorted 64-entry list, one entry per lane, and takes
//                         a partial list in with one bitonic merge: the elementwise better of the list and the
//                         reversed partial list holds the 64 best of both as a bitonic sequence, which six
//                         compare-exchange steps over lane xor 32 .. 1 sort.  The waves share the partial lists, wave
//                         0 merges the 16 results, gathers the winners' score rows and fills the summary.
//
// The order everywhere is the pair (total descending, node ascending), compared as a pair: total is a weighted sum
// whose weights the configuration does not bound to 32 bits.
#pragma once

#include <climits>

#include "ks_device.h"

namespace ks {

constexpr int kSumThreads = 256;                 // nodes per workgroup of summary_block_kernel
constexpr int kSumTop = KS_SUMMARY_MAX_TOP;      // entries of a partial list (its stride, whatever top_n is)
constexpr int kSumBins = 34;                     // the 32 reason bits, feasible nodes, unresolvable nodes
constexpr int kSumBinFeasible = 32, kSumBinUnres = 33;
constexpr int kSumMergeWaves = 16;
constexpr int64_t kSumNoTotal = INT64_MIN;       // the sentinel pair: after every real pair (totals are >= 0)
constexpr int32_t kSumNoNode = INT32_MAX;
static_assert(kSumTop == 64, "a wave holds one list entry per lane");

// what the host copies back in one piece: the summary, then the top rows
struct SumOut {
  ks_pod_summary s;
  int64_t top_totals[kSumTop];
  int64_t top_scores[kSumTop * KS_NUM_SCORE_PLUGINS];
  int32_t top_nodes[kSumTop];
};

__device__ __forceinline__ bool sum_better(int64_t ta, int32_t ia, int64_t tb, int32_t ib) {
  return ta > tb || (ta == tb && ia < ib);
}

__global__ __launch_bounds__(kSumThreads) void summary_block_kernel(int64_t n, const uint32_t* __restrict__ reasons,
                                                                    const int64_t* __restrict__ total, uint32_t mask,
                                                                    int32_t k, uint64_t* __restrict__ fbits,
                                                                    uint64_t* __restrict__ ubits,
                                                                    uint32_t* __restrict__ blk_bins,
                                                                    int64_t* __restrict__ part_tot,
                                                                    int32_t* __restrict__ part_idx, int32_t only) {
  __shared__ uint32_t bins[kSumBins];
  __shared__ int64_t stot[kSumThreads];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * kSumThreads + tid;
  const uint32_t r = i < n ? reasons[i] : 0u;  // (reasons is not padded: no read at or past n)
  // only >= 0 (ks_eval_pod_summary_nominated): the pod's nominated node is the whole feasible set when it is feasible
  // (upstream evaluateNominatedNode); the reason bins and the unresolvable set keep every node's own status
  const bool one = only >= 0 && reasons[only] == 0u;
  const bool feas = i < n && r == 0u && (!one || i == (int64_t)only);
  const bool unres = (r & mask) != 0u;
  const int64_t t = feas ? total[i] : kSumNoTotal;
  if (tid < kSumBins) bins[tid] = 0u;
  stot[tid] = t;
  __syncthreads();
  const uint64_t bf = __ballot(feas), bu = __ballot(unres);
  if (lane == 0) {
    if (i < n) {  // lane 0's node is 64 * word: the word exists iff that node does
      fbits[i >> 6] = bf;
      ubits[i >> 6] = bu;
    }
    if (bf) atomicAdd(&bins[kSumBinFeasible], (uint32_t)__popcll(bf));
    if (bu) atomicAdd(&bins[kSumBinUnres], (uint32_t)__popcll(bu));
  }
  if (__ballot(r != 0u)) {  // (wave-uniform)
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const uint64_t m = __ballot(((r >> b) & 1u) != 0u);
      if (lane == 0 && m) atomicAdd(&bins[b], (uint32_t)__popcll(m));
    }
  }
  const size_t base = (size_t)blockIdx.x * kSumTop;
  if (feas) {
    // the node's position among the workgroup's pairs; nodes ascend with tid, and an infeasible slot never beats
    int rank = 0;
    for (int j = 0; j < kSumThreads; ++j) {
      const int64_t tj = stot[j];
      rank += (tj > t || (tj == t && j < tid)) ? 1 : 0;
    }
    if (rank < k) {
      part_tot[base + rank] = t;
      part_idx[base + rank] = (int32_t)i;
    }
  }
  __syncthreads();
  if (tid < kSumBins) blk_bins[(size_t)blockIdx.x * kSumBins + tid] = bins[tid];
  if (tid < k && (uint32_t)tid >= bins[kSumBinFeasible]) {
    part_tot[base + tid] = kSumNoTotal;
    part_idx[base + tid] = kSumNoNode;
  }
}

// The wave's sorted list (t, ix: one entry per lane, best in lane 0) takes in the list whose entry 63 - lane is
// (tb, ib): the 64 best of both, sorted.  All 64 lanes active.
__device__ __forceinline__ void sum_merge64(int64_t& t, int32_t& ix, int64_t tb, int32_t ib, int lane) {
  if (sum_better(tb, ib, t, ix)) {
    t = tb;
    ix = ib;
  }
#pragma unroll
  for (int j = 32; j >= 1; j >>= 1) {
    const int64_t to = __shfl_xor(t, j, 64);
    const int32_t io = __shfl_xor(ix, j, 64);
    const bool ob = sum_better(to, io, t, ix);
    if ((lane & j) == 0 ? ob : !ob) {  // the lower lane keeps the better pair, the upper lane the other one
      t = to;
      ix = io;
    }
  }
}

__global__ __launch_bounds__(kSumMergeWaves * 64) void summary_merge_kernel(int64_t n, int32_t blocks, int32_t top_n,
                                                                            int32_t k,
                                                                            const uint32_t* __restrict__ blk_bins,
                                                                            const int64_t* __restrict__ part_tot,
                                                                            const int32_t* __restrict__ part_idx,
                                                                            const int64_t* __restrict__ scores,
                                                                            SumOut* __restrict__ out) {
  __shared__ int64_t wtot[kSumMergeWaves][64];
  __shared__ int32_t widx[kSumMergeWaves][64];
  __shared__ uint32_t bins[kSumBins];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the bins: a column per wave at a time, summed over the workgroups' rows (at most n < 2^31 in all)
  for (int c = wave; c < kSumBins; c += kSumMergeWaves) {
    uint32_t v = 0;
    for (int b = lane; b < blocks; b += 64) v += blk_bins[(size_t)b * kSumBins + c];
    v = wave_sum_u32(v);
    if (lane == 0) bins[c] = v;
  }
  int64_t t = kSumNoTotal;
  int32_t ix = kSumNoNode;
  const int rl = 63 - lane;
  for (int b = wave; b < blocks; b += kSumMergeWaves) {
    const bool have = rl < k;  // entries at and past k were not written
    const int64_t tb = have ? part_tot[(size_t)b * kSumTop + rl] : kSumNoTotal;
    const int32_t ib = have ? part_idx[(size_t)b * kSumTop + rl] : kSumNoNode;
    sum_merge64(t, ix, tb, ib, lane);
  }
  wtot[wave][lane] = t;
  widx[wave][lane] = ix;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < kSumMergeWaves; ++w) sum_merge64(t, ix, wtot[w][rl], widx[w][rl], lane);
  const bool row = lane < top_n && ix != kSumNoNode;  // (the sentinels sort last: the rows are lanes 0 .. top_count-1)
  const uint64_t rows = __ballot(row);
  if (row) {
    out->top_nodes[lane] = ix;
    out->top_totals[lane] = t;
    for (int p = 0; p < KS_NUM_SCORE_PLUGINS; ++p)
      out->top_scores[lane * KS_NUM_SCORE_PLUGINS + p] = scores[(size_t)ix * KS_NUM_SCORE_PLUGINS + p];
  }
  if (lane < 32) out->s.reason_nodes[lane] = (int64_t)bins[lane];
  if (lane == 0) {
    out->s.nodes = n;
    out->s.feasible = (int64_t)bins[kSumBinFeasible];
    out->s.unresolvable = (int64_t)bins[kSumBinUnres];
    out->s.best_total = ix != kSumNoNode ? t : -1;
    out->s.best_node = ix != kSumNoNode ? ix : -1;
    out->s.top_count = (int32_t)__popcll(rows);
  }
}

}  // namespace ks
