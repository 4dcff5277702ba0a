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

// ---- the batched queue with a table loaded (ks_schedule_nominated, DESIGN §2.12a "queue") ----
//
//   queue table              built from the host rows at every schedule call, next to the CSR above: per row the seven
//                            request words and a count word (1; 0 once retired) as columns `val`, and their inclusive
//                            prefix sums within the node as columns `pre`.  A node's rows are in descending priority, so
//                            the counted sum for a pod is "binary-search the last row with priority >= the pod's, read
//                            one prefix"; the pod's own row, when it lies inside that range, is subtracted.
//   NomPod                   per staged pod: priority, own nominated node, the index of its own row, owner flag.  An
//                            owner (self_id >= 0 or nominated_node >= 0) is scheduled alone: the commit's pass ends in
//                            front of it, and a pass that starts at it takes that pod only (ks_pass.h, NOM variants).
//   nom_fit_fails            per lane (lane = node): NodeResourcesFit on the node row plus the counted sum.
//   nom_retire_kernel        one wave after each commit: when the pass was an owner's and it reserved, the owner's row is
//                            zeroed and its node's prefix sums rebuilt (lane = column), so no later pod counts it.
constexpr int kNomCols = kNomWords + 1;  // the request words, then the count

struct NomPod {
  int32_t prio;
  int32_t only;   // the pod's own nominated node, tried first (-1 = none)
  int32_t own;    // its own row in the table (-1 = none)
  int32_t owner;  // 1: scheduled alone
};

struct DevNomQueue {
  const int64_t* beg;       // [n + 1], DevNominated's
  const int32_t* prio;      // [m]
  int64_t* val;             // [kNomCols][m]
  int64_t* pre;             // [kNomCols][m]
  const int32_t* row_node;  // [m]
  const NomPod* pods;       // [staged pods]
  int32_t* prev;            // the cursor before the last commit (nom_retire_kernel)
  int64_t m, n;
};

__device__ __forceinline__ NomPod load_nompod_uniform(const NomPod* p) {
  NomPod r;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) int64_t* ConstWords;
  const ConstWords src = (ConstWords)p;
  int64_t* dst = reinterpret_cast<int64_t*>(&r);
  dst[0] = src[0];
  dst[1] = src[1];
#else
  r = *p;
#endif
  return r;
}

// NodeResourcesFit of pod p (nomination w) on node row r with the counted rows of [b, e) added: true = it fails.
// The caller has tested b != e.  Divergent across lanes (each lane its own node), no cross-lane traffic.
// The checks are those of eval_pod_node's Fit (ks_device.h, DEBUG = false) on the row with the sum applied as
// nominated_overlay_kernel applies it; they are written out here on the sum's words so that the node row -- whose score
// terms must stay without the nominated pods -- is not copied per pod in the sweep's loop.  Keep the two in step.
template <int NSC>
__device__ __forceinline__ bool nom_fit_fails(const DevNomQueue& q, const Cfg& c, const NomPod& w, const PodRec& p,
                                              const NodeReg<NSC>& r, int64_t b, int64_t e) {
  if (!c.fit_filter) return false;
  int64_t lo = b, hi = e;  // -> the first row below the pod's priority
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (gld(q.prio + mid) >= w.prio) lo = mid + 1;
    else hi = mid;
  }
  if (lo == b) return false;
  const int64_t last = lo - 1;
  const bool own = (int64_t)w.own >= b && (int64_t)w.own <= last;
  auto sum = [&](int d) -> int64_t {
    int64_t s = gld(q.pre + (int64_t)d * q.m + last);
    if (own) s -= gld(q.val + (int64_t)d * q.m + w.own);
    return s;
  };
  const int64_t cnt = sum(kNomWords);
  if (cnt == 0) return false;
  bool bad = (int64_t)r.pod_count + cnt + 1 > (int64_t)r.allowed;
  if (!(p.flags & kPodAllZero)) {
    bad |= p.cpu > r.free_cpu - sum(0);
    bad |= p.mem > r.free_mem - sum(1);
    bad |= p.eph > r.free_eph - sum(2);
#pragma unroll
    for (int k = 0; k < NSC; ++k)
      if (p.sc[k] != 0) bad |= p.sc[k] > r.free_sc[k] - sum(3 + k);
  }
  return bad;
}

// counters: [12] owner passes (ks_stats.diag[4]), [13] retired rows (ks_stats.diag[5])
// (a template so that the header's includers that never launch it define nothing)
template <int NCOLS = kNomCols>
__global__ __launch_bounds__(64) void nom_retire_kernel(DevNomQueue q, const ks_result* __restrict__ results,
                                                        const int32_t* __restrict__ cursor, unsigned long long* counters) {
  const int lane = threadIdx.x;
  const int32_t c0 = __builtin_amdgcn_readfirstlane(*q.prev), c1 = __builtin_amdgcn_readfirstlane(*cursor);
  if (c1 <= c0) return;  // the pass committed nothing
  if (lane == 0) *q.prev = c1;
  const NomPod w = load_nompod_uniform(q.pods + c0);
  if (!w.owner) return;
  if (lane == 0) atomicAdd(&counters[12], 1ull);
  if (w.own < 0 || w.own >= q.m || __builtin_amdgcn_readfirstlane(results[c0].status) != KS_S_SCHEDULED) return;
  const int64_t node = gld(q.row_node + w.own);
  if (node < 0 || node >= q.n) return;
  const int64_t b = gld(q.beg + node), e = gld(q.beg + node + 1);
  if (lane < NCOLS) {
    int64_t* v = q.val + (int64_t)lane * q.m;
    int64_t* pf = q.pre + (int64_t)lane * q.m;
    gst(v + w.own, (int64_t)0);
    int64_t run = 0;
    for (int64_t i = b; i < e; ++i) {
      run += i == w.own ? 0 : gld(v + i);
      gst(pf + i, run);
    }
  }
  if (lane == 0) atomicAdd(&counters[13], 1ull);
}

}  // namespace ks
