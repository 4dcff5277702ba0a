// ks_plan.h — which commit kernel a context runs and how its LDS image is laid out (host code).
//
// commit_plan() is a pure function of CommitPlanIn: the decisions are taken once, in the order in which they depend on
// one another, and then only read (koordgpu.hip: commit_attr_set computes the plan at every entry point that commits;
// the function attributes, the launches' smem and ks_stats all come from it).  The order: kernel variant, wide-NUMA
// shrink of k, PodStat in LDS, quota rows in LDS, reservation slots (which may evict the quota rows), the image size,
// the dedicated fq kernel and its slot-key table, the mono kernel, Reserve ahead of the commit.
#pragma once

#include <algorithm>

#include "ks_pass.h"
#include "ks_mono.h"

namespace ks {

// Bytes the stat-LDS test, the reservation-slot fit and the k-shrink loop keep free below kLdsBytes; the quota-row
// test and the slot-key table test keep none.  (Kept as found: the code does not say what the 64 bytes stand for.)
constexpr size_t kPlanMargin = 64;

// Kernel variant (FEAT bits, ks_pass.h): 1 Reservation, 2 NodeNUMAResource, 4 the normalized plugins (DeviceShare,
// TaintToleration / NodeAffinity / NodePorts), 8 NUMA topology policies (with 2), 16 reservations holding devices (with
// 1 and 4: DeviceShare's restore state, ks_rsv.h; without it the restore code costs the 7 / 15 kernels ~30 % at c3r,
// though no node runs it).  A context runs the smallest built
// variant whose bits cover the plugins it enables: a bit that is compiled in but unused still costs registers -- the
// variants with Reservation and the normalized plugins together spill 180-320 B/lane in the commit kernel, those
// without Reservation (4, 6, 14) none (hipcc -Rpass-analysis=kernel-resource-usage).
#define KS_FEAT_VALUE(F) F,
constexpr int kBuiltFeats[] = {KS_FEAT_LIST(KS_FEAT_VALUE)};  // ascending
#undef KS_FEAT_VALUE

inline int plan_feat(const Cfg& kc, bool dev_held_any) {
  const int need = (kc.rsv ? 1 : 0) | (kc.numa ? 2 : 0) | ((kc.dev || kc.stat) ? 4 : 0) | (kc.numa_pol ? 10 : 0) |
                   ((kc.rsv && kc.dev && dev_held_any) ? 21 : 0);
  for (int f : kBuiltFeats)
    if ((f & need) == need) return f;
  return 31;
}

struct CommitPlanIn {
  Cfg kc;
  int32_t k_cfg;      // the configured candidates per pod
  int64_t nchunks;
  int nsc;
  int numa_w;         // kNumaDev or kNumaWide
  int32_t q;          // quota rows
  bool dev_held_any;  // a reservation holds devices on some node
  bool commit_fq;     // KS_COMMIT_FQ
  bool fq_keys;       // KS_FQ_KEYS
  int general_mode;   // KS_COMMIT_GENERAL
  bool pre_rsv;       // KS_PRE_RSV
};

enum class PlanStatus {
  kOk,
  kHeldWide,  // reservations holding devices at NUMA width kNumaWide (FEAT 31 is built at width kNumaDev only)
  kTooLarge,  // the general kernel's image exceeds the LDS
};

struct CommitPlan {
  PlanStatus status = PlanStatus::kOk;
  int feat = 0;               // the pass kernels' FEAT variant
  bool wide = false;          // ... at NUMA width kNumaWide
  int32_t k = 0;              // candidates per pod (<= k_cfg)
  bool hint_variant = false;  // the variant runs the helper waves (NUMA policies + DeviceShare compiled in, ks_pass.h)
  bool stat_lds = false;      // CommitArgs.stat_lds
  bool qcache = false;        // quota rows in LDS (the kernels' QC)
  int32_t rcap = 0;           // reservations cached per commit slot
  size_t rsv_bytes = 0, dev_bytes = 0, numa_bytes = 0;  // CommitArgs: the slot regions of the image
  size_t smem = 0;            // the general kernel's image
  size_t smem_no_qcache = 0;  // ... without the quota rows (the topology step's single-pod commit)
  bool hint = false;          // CommitLayout.hint: the helper waves' hints are in the image
  bool fq = false;            // the dedicated Fit + LoadAware + ElasticQuota kernel runs (ks_fq.h), unless patched
  bool fq_keys = false;       // ... with its slot-key table
  size_t fq_smem = 0;         // its image (0 without fq)
  bool mono = false;          // the monotone commit kernel runs (ks_mono.h)
  size_t mono_smem = 0;       // its image (0 where the plugin set or KS_COMMIT_GENERAL rules it out; set when too large)
  bool pre_reserve = false;   // reserve_pre_kernel runs ahead of the commit
};

inline size_t plan_numa_bytes(const CommitPlanIn& in) {
  return in.kc.numa_pol ? (size_t)kMaxBatch * (6 * in.numa_w + 1) * 8 : 0;  // NumaSlotT<numa_w>::kWords per slot
}

// The general commit kernel's layout for this context: the one host call of commit_layout.
// slot_keys: the dedicated fq kernel's image with its slot-key table (FEAT 0, no helper waves).
inline CommitLayout plan_layout(const CommitPlanIn& in, int32_t k, bool qc, size_t rsv_bytes, size_t dev_bytes,
                                bool slot_keys = false) {
  const int feat = plan_feat(in.kc, in.dev_held_any);
  return commit_layout(k, in.nchunks, qc, rsv_bytes, dev_bytes, plan_numa_bytes(in), in.q, slot_keys || feat == 0,
                       !slot_keys && (feat & 12) == 12, slot_keys);
}

inline CommitPlan commit_plan(const CommitPlanIn& in) {
  const Cfg& kc = in.kc;
  CommitPlan p;
  p.feat = plan_feat(kc, in.dev_held_any);
  p.wide = in.numa_w == kNumaWide;
  p.hint_variant = (p.feat & 12) == 12;
  // (unreachable: the loads refuse the combination, dev_apply_held / numa_install)
  if (p.wide && p.feat == 31) p.status = PlanStatus::kHeldWide;
  p.numa_bytes = plan_numa_bytes(in);

  // the slot device region of the commit kernel: GPU state (DeviceShare), then the TaintToleration / NodeAffinity words
  // and NodePorts words (4 x u64 per slot, the region's last kMaxBatch * 32 B) after the pass's PodStat records and the
  // normalization maxima table (ks_pass.h commit_kernel)
  auto dev_bytes = [&](bool stat_lds) {
    return (kc.dev ? (size_t)kDevLdsStride * (kDevTW + kDevQW) * 8 + (size_t)kMaxBatch * 4 : 0) +
           ((kc.dev || kc.stat) ? (size_t)kNormRows * kMaxBatch * 8 : 0) + (kc.stat ? (size_t)kMaxBatch * 32 : 0) +
           (stat_lds ? (size_t)kMaxBatch * sizeof(PodStat) : 0);
  };
  // The pass's PodStat records go to LDS when the commit image still fits with them (before the quota-row and
  // reservation caches are sized); otherwise the commit reads them from HBM (CommitArgs.stat_lds)
  auto stat_lds = [&](int32_t k) {
    return kc.stat && plan_layout(in, k, false, 0, dev_bytes(true)).total + kPlanMargin <= kLdsBytes;
  };

  // A NUMA table at width 8 doubles the slots' NUMA cache (25 KB); next to DeviceShare's slot cache the layout then
  // exceeds the LDS at the default 32 candidates per pod.  Such a context keeps fewer candidates per pod: the
  // placements do not depend on the list length (a pod whose list runs out cuts the pass), only the pass count does.
  p.k = in.k_cfg;
  while (p.wide && p.k > 8 &&
         plan_layout(in, p.k, false, 0, dev_bytes(stat_lds(p.k))).total + kPlanMargin > kLdsBytes)
    p.k -= 8;
  p.stat_lds = stat_lds(p.k);
  p.dev_bytes = dev_bytes(p.stat_lds);

  // Quota rows are cached in LDS for the pass when the table is small enough and the LDS image fits.
  p.qcache = kc.quota_enable && in.q > 0 && in.q <= kQuotaLdsRows &&
             plan_layout(in, p.k, true, 0, p.dev_bytes).total <= kLdsBytes;

  // Reservations cached per commit slot: as many as fit next to the rest of the commit layout (<= 8);
  // the quota-row cache yields to it when both do not fit.
  const size_t rsv_rec = (size_t)kMaxBatch * 8 * (size_t)(3 + 2 * (3 + in.nsc) + 2);  // sizeof(RsvRec<3+nsc>) per slot
  if (kc.rsv) {
    auto fit = [&](bool qc) {
      const size_t base = plan_layout(in, p.k, qc, 0, p.dev_bytes).total + kPlanMargin;
      const size_t avail = base < kLdsBytes ? kLdsBytes - base : 0;
      return (int32_t)std::min<size_t>(8, avail / rsv_rec);
    };
    p.rcap = fit(p.qcache);
    if (p.qcache && p.rcap < 4) {
      p.qcache = false;
      p.rcap = fit(false);
    }
  }
  p.rsv_bytes = rsv_rec * p.rcap;

  const CommitLayout L = plan_layout(in, p.k, p.qcache, p.rsv_bytes, p.dev_bytes);
  p.smem = L.total;
  p.hint = L.hint;
  if (p.smem > kLdsBytes && p.status == PlanStatus::kOk) p.status = PlanStatus::kTooLarge;
  // (the reservation cache that fit next to the quota rows fits without them)
  p.smem_no_qcache = p.qcache ? plan_layout(in, p.k, false, p.rsv_bytes, p.dev_bytes).total : p.smem;

  // The dedicated commit kernel of the monotone Fit (LeastAllocated) + LoadAware + ElasticQuota plugin set (ks_fq.h)
  // runs exactly where commit_kernel<NSC, true, 0> would run for a monotone profile: quota tables in LDS, no
  // Reservation / NUMA / DeviceShare / dictionary plugins, not the patched pipeline (its lists can hold emptied
  // chunks and its tops are rebuilt: the launch tests that per run).  KS_COMMIT_FQ=0, read when the context is created,
  // keeps the general kernel (A/B, tests).  Same CommitArgs and LDS layout as the general kernel.
  p.fq = in.commit_fq && p.qcache && p.feat == 0 && kc.monotone && !kc.fit_most && kc.quota_enable;

  // The dedicated kernel's slot-key table (ks_fq.h, KEYS = true): a slow pod's keys on the touched slots come from the
  // evaluator wave's LDS table instead of wave 0's own lane = slot evaluation.  On when the commit image still fits the
  // CU's LDS with the table (C2: candidates = 32; not with candidates = 64); otherwise, and with KS_FQ_KEYS=0 (read
  // when the context is created: A/B, tests), wave 0 evaluates as before.  fq_smem: the image with the table.
  if (p.fq) {
    const size_t t = plan_layout(in, p.k, true, 0, p.dev_bytes, true).total;
    p.fq_keys = in.fq_keys && t <= kLdsBytes;
    p.fq_smem = p.fq_keys ? t : p.smem;
  }

  // The monotone commit kernel (ks_mono.h) runs the passes of a plugin set without Reservation, NodeNUMAResource or
  // DeviceShare whose keys commits can only lower (Fit LeastAllocated + LoadAware) when its LDS fits.  With
  // ElasticQuota the general kernel's pass runs instead (as ks_fq.h's dedicated kernel when the quota tables fit the
  // LDS, fq above): its admission look-ahead for pod j + 1 overlaps pod j's Reserve,
  // and that measured faster than the mono kernel's prebuilt rows at C2 (MI355X, commit 20.6 vs 21.4 ms/step;
  // C5 without quota: mono 275.6 vs general 281.3 ms per 200k pods, profiles/r02_commit_ab.txt).
  // KS_COMMIT_GENERAL=1 keeps the general kernel, =2 forces the mono kernel with quota too (A/B).  ks_assume always
  // uses the general kernel.
  if (in.general_mode != 1 && p.feat == 0 && kc.monotone && !kc.fit_most && !(in.general_mode == 0 && kc.quota_enable)) {
    p.mono_smem = mono_layout(p.k, in.nchunks, p.qcache, in.q).total;
    p.mono = p.mono_smem <= kLdsBytes;
  }

  // Reserve's NodeNUMAResource / DeviceShare allocations ahead of the commit (reserve_pre_kernel): on for
  // the NUMA topology policy variants when policy nodes are loaded; KS_PRE_RSV=0 turns it off (A/B).
  p.pre_reserve = in.pre_rsv && kc.numa_pol;
  return p;
}

}  // namespace ks
