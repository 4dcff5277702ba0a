// ks_numa_wide.h — the NUMA topology policy path (ks_numa.h) on nodes with up to kNumaWide = 8 NUMA nodes.
//
// The same FilterByNUMANode -> Admit -> allocateResources -> Score as numa_policy_eval_narrow, with the state that
// does not stretch from 4 to 8 NUMA nodes restated:
//   * the IterateBitMasks order of the 255 masks comes from a compile-time table (ks_numa_masks.h) instead of one
//     64-bit constant;
//   * a hint list is a 256-bit set of positions in that order (4 x u64) plus a flag for "the list is one nil entry";
//   * the per-mask hint scores are not stored: a mask's score is recomputed from the per-NUMA totals when the merge
//     needs it (once per entry of the first list; for the second list only when its mask is the merged mask and the
//     update rule reads the score);
//   * the merge is the walk over cpu list x memory list x DeviceShare's list in product order, first list outermost,
//     with mergeFilteredHints' order-dependent update rule (up to 255 x 255 x 3 permutations), reduced exactly to
//     the preferred permutations when one exists (see the merge below);
//   * tryBestToDistributeEvenly's positional insertion sort, splitQuantity, allocateCPUSet's counts and the score
//     sums run over 8 entries, "select by compare" instead of indexed arrays (those would live in scratch memory).
// DeviceShare's hints are the narrow path's (DevHints over at most 2 device NUMA ids on nodes with at most 2 NUMA
// nodes): a wide context still holds 2-NUMA GPU policy nodes.
// Included by ks_numa.h (after the narrow path); not a header of its own.
#pragma once

#include "ks_numa_masks.h"

namespace ks {

[[maybe_unused]] static __constant__ NumaMaskOrder kNumaMaskOrder = make_numa_mask_order();

__device__ __forceinline__ uint32_t numa_wide_mask_at(int K, int i) { return (uint32_t)kNumaMaskOrder.m[K][i]; }

// a NodeNUMAResource hint list after filterProvidersHints: positions in the mask order, or one nil entry
struct NumaHintList {
  uint64_t w[4];
  bool nil;
};

__device__ __forceinline__ bool numa_hl_any(const NumaHintList& l) { return l.nil || (l.w[0] | l.w[1] | l.w[2] | l.w[3]) != 0; }

// the list's first entry at or after `from`: a position < 255, 256 = the nil entry, 257 = none
__device__ __forceinline__ int numa_hl_next(const NumaHintList& l, int from) {
  int e = (l.nil && from <= 256) ? 256 : 257;
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const int lo = from - 64 * q;
    const uint64_t x = lo >= 64 ? 0ull : (lo <= 0 ? l.w[q] : ((l.w[q] >> lo) << lo));
    if (x) e = 64 * q + __builtin_ctzll(x);
  }
  return e;
}

template <bool DEFER_DEV = false, typename V, typename DV, typename DHF = NoDevHints>
__device__ __forceinline__ NumaPolOutT<kNumaWide> numa_policy_eval_wide(const Cfg& c, const PodRec& p, const V& v,
                                                                        const NumaNodeCtx& nc, const DV* dv,
                                                                        DHF dhf = DHF{}) {
  constexpr int W = kNumaWide;
  constexpr bool LATE = LateDevHints<DHF>::value;
  NumaPolOutT<W> o;
  o.reasons = 0;
  o.score = 0;
  o.affinity = 0;
  o.admitted = false;
  o.dev_done = o.dev_hit = false;
  o.dev = DevOut{0u, 0, 0u, 0u};
#pragma unroll
  for (int k = 0; k < W; ++k) {
    o.alloc[0][k] = o.alloc[1][k] = 0;
    o.cpus[k] = 0;
  }
  const int K = v.count();
  if (K == 0) {
    o.reasons = KS_R_NUMA_MISSING;
    return o;
  }
  DevHints dh;
  dh.lists = 0;
  dh.npos = 0;
  dh.id0 = dh.id1 = 0;
  dh.ok = 0;
  dh.minaff = -1;
  if (!LATE && dv) dh = dev_hints(c, p, *dv);
  const int pol = v.policy();
  const uint32_t pres = v.present();
  // requestCPUBind / getCPUBindPolicy on this node (as numa_policy_eval_narrow)
  const uint32_t label = c.cores ? cores_label(nc.cores) : 0u;
  const bool pbind = c.cpuset && (p.flags & KS_POD_CPU_BIND);
  const bool bind = pbind || (label != 0u && p.cpu > 0);
  const uint32_t rpol = label ? label
                              : ((pbind && (p.cpu_bind & KS_CPU_BIND_REQUIRED)) ? (p.cpu_bind & KS_CPU_BIND_POLICY_MASK) : 0u);
  const int32_t cpc = max((int32_t)cores_cpc(nc.cores), 1);
  auto used_of = [&](int r, int k) -> int64_t {
    return (k < K && ((pres >> k) & 1u)) ? v.used(r, k) + (r == 0 ? v.off(k) : 0) : 0;
  };
  int64_t tot[2][W], av[2][W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      tot[r][k] = k < K ? v.total(r, k) : 0;
      const int64_t a = tot[r][k] - used_of(r, k);
      av[r][k] = a < 0 ? 0 : a;
    }
    // trimNUMANodeResources (resource_manager.go:144-167)
    if (rpol && k < K && av[0][k] != 0) {
      const int64_t fk = (int64_t)numa_filtered(v.freew(k), rpol, cpc) * 1000;
      if (fk < av[0][k]) av[0][k] = fk;
    }
  }
  const int64_t req_cpu = (bind && nc.ratio > 1.0) ? (int64_t)::ceil((double)p.cpu * nc.ratio) : p.cpu;
  const int64_t req[2] = {req_cpu, p.mem};
  const bool want[2] = {p.cpu != 0, p.mem != 0};
  const int nm = (1 << K) - 1;
  uint32_t lack[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < W; ++k)
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (k < K && av[r][k] == 0) lack[r] |= 1u << k;
  const bool nmost = c.numa_sc_most != 0;
  // the hint score of a mask (the NUMAScoringStrategy scorer over its NUMA nodes), recomputed on demand
  auto mask_score = [&](uint32_t mk) -> int32_t {
    int64_t ts[2] = {0, 0}, fs[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < W; ++k)
      if ((mk >> k) & 1u)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          ts[r] += tot[r][k];
          fs[r] += av[r][k];
        }
    return numa_res_score(c, nmost, ts[0] - fs[0], ts[1] - fs[1], ts[0], ts[1], req[0], req[1]);
  };
  // NodeNUMAResource hints: bit i of hs[r] = mask i is a hint of resource r
  NumaHintList hs[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    hs[r].w[0] = hs[r].w[1] = hs[r].w[2] = hs[r].w[3] = 0;
    hs[r].nil = false;
  }
  int min_size[2] = {K, K};
  for (int i = 0; i < nm; ++i) {
    const uint32_t mk = numa_wide_mask_at(K, i);
    int64_t ts[2] = {0, 0}, fs[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < W; ++k)
      if ((mk >> k) & 1u)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          ts[r] += tot[r][k];
          fs[r] += av[r][k];
        }
    const int cnt = __builtin_popcount(mk);
    const uint64_t bit = 1ull << (i & 63);
    const int wi = i >> 6;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!want[r] || ts[r] < req[r] || (mk & lack[r])) continue;
      min_size[r] = cnt < min_size[r] ? cnt : min_size[r];
      if (fs[r] >= req[r]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) hs[r].w[q] |= wi == q ? bit : 0ull;
      }
    }
  }
  const bool single = pol == KS_NUMA_POLICY_SINGLE_NUMA_NODE;
  // The lists after filterProvidersHints (and filterSingleNumaHints).  A list holding only a preferred nil entry (a
  // provider / resource without preference) is a no-op in mergePermutation, so it stands for "no list".  Lists,
  // outermost first: NodeNUMAResource cpu, memory, then DeviceShare (one list, as in the narrow path).
  bool lnp[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    lnp[r] = !want[r];
    const bool none = (hs[r].w[0] | hs[r].w[1] | hs[r].w[2] | hs[r].w[3]) == 0;
    if (!want[r]) {
      hs[r].nil = true;  // no hints for this resource
    } else if (none) {
      hs[r].nil = !single;  // {nil, false}: "no possible NUMA affinities" (filterSingleNumaHints drops it)
    } else if (single) {
      // the preferred single-NUMA-node hints: the size-1 masks are positions 0..K-1 of the order
      hs[r].w[0] = min_size[r] == 1 ? (hs[r].w[0] & ((1ull << K) - 1ull)) : 0ull;
      hs[r].w[1] = hs[r].w[2] = hs[r].w[3] = 0;
    }
  }
  if constexpr (LATE) {
    if (dv) dh = dhf();
  }
  constexpr int kNil = 15;
  uint32_t db = 1u << kNil;
  bool dnp = true;
  if (dh.lists) {
    dnp = false;
    if (dh.ok == 0) {
      db = single ? 0u : (1u << kNil);  // no allocating mask: {nil, false}
    } else {
      db = 0;
      for (int i = 0; i < dh.npos; ++i) {
        if (!((dh.ok >> i) & 1u)) continue;
        const int pc = __builtin_popcount(dev_hint_mask(dh, i));
        if (!single || (pc == 1 && pc == dh.minaff)) db |= 1u << i;
      }
    }
  }
  // mergeFilteredHints over the cartesian product, first list outermost (policy.go:129-226)
  const uint32_t dflt = (1u << K) - 1u;
  uint32_t best_mask = dflt;
  bool best_pref = false;
  int32_t best_score = 0;
  // Exact reduction of the walk.  The first preferred permutation replaces whatever the non-preferred ones before it
  // left, and from then on only preferred ones are looked at; so when one exists the result is the fold over the
  // preferred permutations alone, in product order.  A preferred permutation has equal masks in every list that has
  // one, so with a cpu hint m0 the only memory entries that can make one are the same position of the memory list or
  // its nil entry: walk 0 visits just those (at most 255 x 1 x 3 permutations) and skips the non-preferred ones.
  // Walk 1, the full product, runs only when walk 0 found none -- then every permutation is non-preferred and the
  // state is still the initial one -- and only under best-effort: restricted and single-numa-node admit nothing
  // without a preferred hint.
  const bool lists_ok = numa_hl_any(hs[0]) && numa_hl_any(hs[1]) && db;
  for (int walk = 0; lists_ok && walk < 2 && !best_pref && (walk == 0 || pol == KS_NUMA_POLICY_BEST_EFFORT); ++walk) {
    for (int e0 = numa_hl_next(hs[0], 0); e0 <= 256; e0 = numa_hl_next(hs[0], e0 + 1)) {
      const uint32_t m0 = e0 == 256 ? 0u : numa_wide_mask_at(K, e0);
      const bool h0 = e0 == 256 ? lnp[0] : __builtin_popcount(m0) == min_size[0];
      const int32_t s0 = e0 == 256 ? 0 : mask_score(m0);
      const bool pin = walk == 0 && m0 != 0u;  // (a list holds positions or the nil entry, never both)
      const int e1_first = !pin ? numa_hl_next(hs[1], 0)
                                : (numa_hl_next(hs[1], e0) == e0 ? e0 : (hs[1].nil ? 256 : 257));
      for (int e1 = e1_first; e1 <= 256; e1 = pin ? 257 : numa_hl_next(hs[1], e1 + 1)) {
        const uint32_t m1 = e1 == 256 ? 0u : numa_wide_mask_at(K, e1);
        const bool h1 = e1 == 256 ? lnp[1] : __builtin_popcount(m1) == min_size[1];
        for (uint32_t b2 = db; b2; b2 &= b2 - 1u) {
          const int e2 = __builtin_ctz(b2);
          const uint32_t m2 = e2 == kNil ? 0u : dev_hint_mask(dh, e2);
          const bool h2 = e2 == kNil ? dnp : __builtin_popcount(m2) == dh.minaff;
          // mergePermutation
          uint32_t merged = dflt, first = 0;
          bool pref = h0 && h1 && h2, have = false;
          if (m0) { first = m0; have = true; merged &= m0; }
          if (m1) { if (have && m1 != first) pref = false; if (!have) first = m1; have = true; merged &= m1; }
          if (m2) { if (have && m2 != first) pref = false; have = true; merged &= m2; }
          if (merged == 0 || (walk == 0 && !pref)) continue;
          // the merged hint's score: the highest of the NodeNUMAResource hints whose mask is the merged mask
          auto msc_of = [&]() -> int32_t {
            int32_t msc = 0;
            if (m0 == merged && s0 > msc) msc = s0;
            if (m1 == merged) {
              const int32_t s1 = mask_score(m1);
              if (s1 > msc) msc = s1;
            }
            return msc;
          };
          if (pref && !best_pref) {
            best_score = msc_of(); best_mask = merged; best_pref = true;
          } else if (!pref && best_pref) {
          } else if (!numa_narrower(merged, best_mask)) {
            if (__builtin_popcount(merged) == __builtin_popcount(best_mask)) {
              const int32_t msc = msc_of();
              if (msc > best_score) { best_mask = merged; best_pref = pref; best_score = msc; }
            }
          } else {
            best_score = msc_of(); best_mask = merged; best_pref = pref;
          }
        }
      }
    }
  }
  uint32_t affinity = best_mask;
  bool admit = true;
  if (single) {
    if (affinity == dflt) affinity = 0u;
    admit = best_pref;
  } else if (pol == KS_NUMA_POLICY_RESTRICTED) {
    admit = best_pref;
  }
  if (!admit) {
    o.reasons = KS_R_NUMA_AFFINITY;
    return o;
  }
  o.admitted = true;
  o.affinity = affinity;
  // the NUMA plugin's Allocate (tryBestToDistributeEvenly)
  if (affinity) {
    const int nb = __builtin_popcount(affinity);
    int ord0[W];  // the affinity's NUMA ids ascending
    {
      uint32_t b = affinity;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        ord0[i] = b ? __builtin_ctz(b) : 0;
        b &= b - 1u;
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!want[r]) continue;
      int ord[W];
#pragma unroll
      for (int i = 0; i < W; ++i) ord[i] = ord0[i];
      // sort.Slice insertion sort with less(i, j) comparing totalAvailable by slice position (fixed per position)
#pragma unroll
      for (int i = 1; i < W; ++i) {
        bool go = i < nb;
#pragma unroll
        for (int j = i; j > 0; --j) {
          const int64_t aj = j < K ? av[r][j] : 0, ai = (j - 1) < K ? av[r][j - 1] : 0;
          go = go && aj < ai;
          if (go) {
            const int t = ord[j];
            ord[j] = ord[j - 1];
            ord[j - 1] = t;
          }
        }
      }
      int64_t q = r == 0 ? p.cpu : p.mem;  // originalRequests
#pragma unroll
      for (int i = 0; i < W; ++i) {
        if (i >= nb) break;
        // splitQuantity (:285-300)
        int64_t split = q / (nb - i);
        if (r == 0 && bind)
          split = rpol == KS_CPU_BIND_FULL_PCPUS ? ((q + 999) / 1000) / cpc / (nb - i) * cpc * 1000
                                                 : ((q + 999) / 1000) / (nb - i) * 1000;
        int64_t a = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) a = ord[i] == k ? av[r][k] : a;
        const int64_t got = a > split ? split : a;
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (ord[i] == k) o.alloc[r][k] = got;
        q -= got;
      }
      if (q != 0) {
        o.reasons = KS_R_NUMA_INSUFFICIENT;
        return o;
      }
    }
  }
  bool any_alloc = false;
#pragma unroll
  for (int k = 0; k < W; ++k) any_alloc |= o.alloc[0][k] != 0 || o.alloc[1][k] != 0;
  if (bind) {
    // allocateCPUSet (:314-401), as numa_policy_eval_narrow
    const int32_t need = pbind ? (int32_t)(p.cpu_bind >> 8) : (int32_t)(p.cpu / 1000);
    const int32_t have = !rpol ? nc.cpu_free
                               : (rpol == KS_CPU_BIND_FULL_PCPUS ? (int32_t)cores_full(nc.cores) * cpc
                                                                 : (int32_t)cores_any(nc.cores));
    if (nc.cpu_free < 0 || have < need) {
      o.reasons = KS_R_NUMA_CPUSET;
      return o;
    }
    if (any_alloc) {
      int32_t taken = 0;
      bool whole = true;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if (o.alloc[0][k] == 0 && o.alloc[1][k] == 0) continue;
        const int32_t f = rpol ? numa_filtered(v.freew(k), rpol, cpc) : v.freec(k), w = (int32_t)(o.alloc[0][k] / 1000);
        o.cpus[k] = f < w ? f : w;
        taken += o.cpus[k];
        whole = whole && (o.cpus[k] % cpc == 0);
      }
      if (taken != need || (rpol == KS_CPU_BIND_FULL_PCPUS && !whole)) {
        o.reasons = KS_R_NUMA_CPUSET;
        return o;
      }
    }
  }
  // DeviceShare's Allocate with the affinity (with DEFER_DEV the caller's DeviceShare Filter, same restriction)
  if (dv) {
    o.dev_done = true;
    if (!DEFER_DEV) {
      o.dev = dev_eval<false>(c, p, *dv, nullptr, affinity ? affinity : ~0u);
      o.dev_hit = true;
      if (o.dev.reasons) {
        o.reasons = o.dev.reasons;
        return o;
      }
    }
  }
  int64_t trq[2] = {0, 0}, tal[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (o.alloc[0][k] == 0 && o.alloc[1][k] == 0) continue;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      tal[r] += tot[r][k];
      trq[r] += used_of(r, k);
    }
  }
  if (!any_alloc) {
    trq[0] = nc.plain_req_cpu;
    trq[1] = nc.plain_req_mem;
    tal[0] = nc.plain_alloc_cpu;
    tal[1] = nc.plain_alloc_mem;
  }
  if (bind) trq[0] = nc.cs_milli + nc.cs_off;  // Amplify(allocated cpuset CPUs x 1000)
  o.score = numa_res_score(c, c.numa_most != 0, trq[0], trq[1], tal[0], tal[1], req[0], req[1]);
  return o;
}

}  // namespace ks
