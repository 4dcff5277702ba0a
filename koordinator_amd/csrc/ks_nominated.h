// ks_nominated.h — nominated pods in one pod's Filter (upstream RunFilterPluginsWithNominatedPods / addNominatedPods,
// kube-scheduler v1.24 framework/runtime/framework.go; not on disk: parity unpinned).
//
// A preemptor that ks_preempt nominated to a node (KS_P_NOMINATED) is not on that node yet: the victims are gone, the
// room is free, and the nomination is all that keeps another pod from taking it.  Upstream runs the Filters of pod P on
// node X twice when X has nominated pods of priority >= P's (P itself excluded): once on a NodeInfo copy with them added
// (AddPodInfo: Requested, every scalar and the pod count go up), and, if that passes, once without.  Within the plugin
// set the library admits a nominated table for, only NodeResourcesFit reads what AddPodInfo changes, and it can only
// fail more often with the pods added, so the node's status is the status of the pass with them: the node's own reasons
// with Fit's bits of that pass OR-ed in.
//
//   table                    CSR by node in HBM (ks_load_nominated): beg [n + 1], then per entry -- a node's entries in
//                            descending priority -- priority, id and the seven request words as SoA columns; `nodes`
//                            lists the nodes that have entries.  A node without entries costs one compare of two
//                            adjacent offsets.
//   nominated_sum            one wave: the node's entries strided over the 64 lanes, the entries with
//                            priority >= who's and id != who's own summed per request word and counted, reduced with
//                            the DPP row steps + readlane of ks_device.h.  Used by the overlay kernel and, once per
//                            node, by preempt_dry_run_kernel (ks_preempt.h).
//   nominated_overlay_kernel one wave per nominated node: the node row as the evaluation loads it (load_node), the sum
//                            added the way a Reserve adds a pod to the row, eval_pod_node's Filter on that, and the
//                            Fit bits of its reasons written to the node's word of a zeroed [n] array.  eval_debug_kernel
//                            ORs that word into the node's reasons before anything is derived from them.
#pragma once

#include "ks_device.h"

namespace ks {

constexpr int kNomWords = 3 + KS_MAX_SCALARS;  // cpu, memory, ephemeral-storage, scalar[k]: NodeInfo.Requested's words
constexpr uint32_t kNomFitBits = KS_R_FIT_PODS | KS_R_FIT_CPU | KS_R_FIT_MEMORY | KS_R_FIT_EPHEMERAL | KS_R_FIT_SCALAR;

struct DevNominated {
  const int64_t* beg;    // [n + 1] a node's entries are [beg[i], beg[i + 1]); null = no table
  const int32_t* prio;   // [m] descending within a node
  const int64_t* id;     // [m] the caller's key of the pod
  const int64_t* req;    // [kNomWords][m]
  const int32_t* nodes;  // [nn] the nodes with entries, ascending
  int64_t m;             // stride of req's columns
  int32_t nn;
};

// whose Filter runs: entries below its priority and its own entry do not count
struct NomWho {
  int64_t self_id;  // -1 = none
  int32_t prio;
};

struct NomSum {
  int64_t req[kNomWords];
  int32_t count;
};

// sum over the wave, wave-uniform (the exchange pattern of wave_sum_u32).  All 64 lanes active.
__device__ __forceinline__ int64_t nom_wave_sum_i64(int64_t x) {
  uint64_t v = (uint64_t)x;
  v += dpp64<0xB1>(v);
  v += dpp64<0x4E>(v);
  v += dpp64<0x141>(v);
  v += dpp64<0x140>(v);
  return (int64_t)(readlane64(v, 0) + readlane64(v, 16) + readlane64(v, 32) + readlane64(v, 48));
}

// The nominated pods that count for `who` on `node`, summed.  Called by a whole converged wave; the result is
// wave-uniform.  node < n (beg has n + 1 entries).
__device__ __forceinline__ NomSum nominated_sum(const DevNominated& t, int64_t node, const NomWho& who, int lane) {
  NomSum s{};
  const int64_t b = gld(t.beg + node), e = gld(t.beg + node + 1);
  if (b == e) return s;
  int64_t v[kNomWords] = {};
  uint32_t c = 0;
  for (int64_t i = b + lane; i < e; i += 64) {
    if (gld(t.prio + i) < who.prio) break;  // descending: the rest of this lane's entries are lower still
    if (gld(t.id + i) == who.self_id) continue;
#pragma unroll
    for (int d = 0; d < kNomWords; ++d) v[d] += gld(t.req + (int64_t)d * t.m + i);
    ++c;
  }
#pragma unroll
  for (int d = 0; d < kNomWords; ++d) s.req[d] = nom_wave_sum_i64(v[d]);
  s.count = (int32_t)wave_sum_u32(c);
  return s;
}

template <int NSC>
__global__ __launch_bounds__(256) void nominated_overlay_kernel(DevNominated t, DevNodes d, Cfg c, const PodRec* pod,
                                                                NomWho who, uint32_t* __restrict__ fit_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= t.nn) return;
  const int64_t node = gld(t.nodes + w);
  const NomSum s = nominated_sum(t, node, who, lane);
  if (s.count == 0) return;  // (fit_bits is zeroed before the launch)
  const PodRec p = load_pod_uniform(pod);
  NodeReg<NSC> r;
  load_node<NSC>(c, d, node, 1, r);
  // NodeInfo.AddPodInfo of the counted pods: what reserve_row does to the words the Filter reads
  r.free_cpu -= s.req[0];
  r.free_mem -= s.req[1];
  r.free_eph -= s.req[2];
#pragma unroll
  for (int k = 0; k < NSC; ++k) r.free_sc[k] -= s.req[3 + k];
  r.pod_count += s.count;
  r.pods_full = ((int64_t)r.pod_count + 1 > (int64_t)r.allowed) || !r.valid;
  const EvalOut o = eval_pod_node<NSC, true>(c, p, r);
  if (lane == 0) fit_bits[node] = o.reasons & kNomFitBits;
}

}  // namespace ks
