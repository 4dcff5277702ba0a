// ks_fq.h — the commit kernel of one plugin set: NodeResourcesFit (LeastAllocated) + LoadAwareScheduling +
// ElasticQuota with the quota tables in LDS, a monotone profile (the record bench.py prints).
//
// Same pass as commit_kernel<NSC, true, 0> (ks_pass.h): same CommitArgs, same LDS layout
// (commit_layout), same results, counters, write-back, pipe_* hooks and topology handling, and the same wave-1
// slot-row builder.  What it leaves out is everything the general template carries for the other plugin sets:
//  * only the Cfg words this profile reads are pinned in SGPRs (Fit / LoadAware switches and weights,
//    quota_parent); the rest of Cfg is a compile-time zero;
//  * a pod's scalars (quota row, its parent and masks, the pod's quota mask and flags, candidate count, bound,
//    top key, second-best node) are one 32-byte LDS record, read with two 16-byte broadcast reads in the
//    look-ahead's batch of LDS reads, instead of eight lane-held values and their v_readlanes; Reserve uses what the
//    look-ahead read;
//  * a monotone profile's fast pod (snapshot-best node untouched) always opens a new slot from the prefetched top
//    row, so it skips the slot search; a slow pod's new slot can only be its second-best node or a miss;
//  * no Reservation / NUMA / DeviceShare / dictionary state, no normalization, no cpu-bind Reserve, no ks_assume.
//
// KEYS = true (the slot-key table fits the LDS): a slow pod's keys on the touched slots are not evaluated
// by wave 0 (lane = slot, one full evaluation's latency per slow pod) but ahead of time by the helper waves: whenever
// a slot row changes, one of them evaluates that one row for every pod of the pass (lane = pod) into
// skey[slot][pod].  Waves 1 and 2 share the descriptor queue by entry (even / odd); the one that takes a new slot's
// descriptor builds the row from the prefetched raw row and evaluates it at once (one hand-off), each has its own
// `handled` counter.  Wave 0's slow path is then a wait for both counters, one LDS read and the wave max.
#pragma once

#include "ks_pass.h"

namespace ks {

struct __attribute__((aligned(16))) FqPod {
  uint32_t qmeta;   // the leaf quota row's parent (0xFFFF = none) | limit_mask << 16 | min_mask << 24
  uint32_t flags;   // PodRec.flags
  uint32_t qword;   // quota row (0xFFFF = none) | the pod's quota dimension mask << 16 | candidate count << 24
  int32_t second;   // node of the pod's second-best key (-1 = none)
  uint64_t bound, top;
};
static_assert(sizeof(FqPod) == 32, "FqPod layout");
// the records live in the general layout's per-slot NUMA words (kMaxBatch x 32 B), which this plugin set never uses
static_assert(kMaxBatch == 64 && kMaxCand <= 64 && kQuotaLdsRows < 0xFFFF && KS_QUOTA_DIMS <= 8, "FqPod packing");

// The FqPod words that depend on the pod and the loaded quota table only: written once per ks_schedule_staged call for
// every pod of the queue (prep_fq_words_kernel, koordgpu.hip), read by the select kernel.
__device__ __forceinline__ uint2 fq_step_words(int32_t quota, uint32_t pmask, const DevQuotas& q) {
  uint32_t qmeta = 0xFFFFu;
  if (quota >= 0) {
    const int32_t pp = q.parent[quota];
    qmeta = (uint32_t)(pp < 0 ? 0xFFFF : pp) | ((q.limit_mask[quota] & 0xFFu) << 16) | ((q.min_mask[quota] & 0xFFu) << 24);
  }
  return make_uint2(qmeta, (uint32_t)(quota < 0 ? 0xFFFF : quota) | ((pmask & 0xFFu) << 16));
}

// One pod of a pass as the commit loads it (the staged prologue): the finished FqPod, then the raw rows of the pod's
// snapshot-best and second-best nodes (zero rows where the node is absent).  Written by select_kernel for the pods at
// the cursor it read, record p = pod cursor + p, and copied to precs / rawtop / rawrun by a commit at the same cursor.
struct __attribute__((aligned(16))) FqPassRec {
  FqPod pod;
  int64_t top[32], run[32];
};
static_assert(sizeof(FqPassRec) == 544 && RF_N == 32, "FqPassRec layout");

// 16 bytes as a native vector (arrays of it stay in registers; HIP's uint4 is a struct around a union)
typedef uint32_t Quad __attribute__((ext_vector_type(4)));

// A prologue copy in two halves, so that the loads of several copies are all in flight before the first LDS store.
// No branch around a load (an index past the end re-reads element 0): n >= 1, n <= N * NT.
template <int N, int NT, typename T>
struct ProCopy {
  T v[N];
  __device__ __forceinline__ void issue(const T* src, int32_t n, int tid) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int32_t i = tid + u * NT;
      v[u] = src[i < n ? i : 0];
    }
  }
  __device__ __forceinline__ void store(T* dst, int32_t n, int tid) const {
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int32_t i = tid + u * NT;
      if (i < n) dst[i] = v[u];
    }
  }
};

// rescan_untouched for this kernel: the node-column pointers are re-read per rescan through an opaque pointer, so
// the compiler cannot hoist them into SGPRs for the whole loop (rescans are rare)
template <int NSC>
__device__ __forceinline__ uint64_t fq_rescan(const DevNodes* dnp, const Cfg& cfg, const PodRec& pod, int64_t chunk,
                                              uint64_t touched_mask, int64_t n) {
  const int lane = threadIdx.x & 63;
  const int64_t node = chunk * 64 + lane;
  asm volatile("" : "+s"(dnp));
  const DevNodes d = *dnp;
  NodeReg<NSC> r;
  load_node<NSC>(cfg, d, node, node < n, r);
  const EvalOut o = eval_pod_node<NSC, false>(cfg, pod, r);
  const bool skip = o.reasons || ((touched_mask >> lane) & 1ull);
  return wave_max_u64(skip ? 0ull : gkey(o.total, node));
}

template <int NSC, bool KEYS>
__global__ __launch_bounds__(commit_threads(0)) void commit_fq_kernel(CommitArgs a) {
  constexpr int NT = commit_threads(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int32_t K = a.k;
  const CommitLayout lay = commit_layout(K, a.nchunks, true, (size_t)a.rsv_bytes, (size_t)a.dev_bytes, (size_t)a.numa_bytes,
                                         a.q.q, true, false, KEYS);
  SlotRow* rows = reinterpret_cast<SlotRow*>(smem_raw + lay.rows);
  PodRec* spods = reinterpret_cast<PodRec*>(smem_raw + lay.pods);
  ks_result* sres = reinterpret_cast<ks_result*>(smem_raw + lay.res);
  int64_t* raw = reinterpret_cast<int64_t*>(smem_raw + lay.raw);
  int64_t* rawtop = reinterpret_cast<int64_t*>(smem_raw + lay.rawtop);
  int64_t* rawrun = reinterpret_cast<int64_t*>(smem_raw + lay.rawrun);
  int64_t* pqreq = reinterpret_cast<int64_t*>(smem_raw + lay.pqreq);
  uint2* cand_t = reinterpret_cast<uint2*>(smem_raw + lay.cand_t);
  uint32_t* cand_chunk = reinterpret_cast<uint32_t*>(smem_raw + lay.cand_chunk);
  FqPod* precs = reinterpret_cast<FqPod*>(smem_raw + lay.snuma);
  QuotaRowsLds qview = quota_lds(smem_raw + lay.quota, a.q.q);
  QuotaRowsLds* qlds = &qview;
  unsigned long long* touched = reinterpret_cast<unsigned long long*>(smem_raw + lay.touched);
  // [issue order] {node, slot | pod << 8 | second << 16 | built << 17}: one descriptor per row change.  Without
  // `built` the slot is new and its row was prefetched (rawtop / rawrun): a helper wave builds it and sets its ready
  // bit.  `built` (KEYS only): the row is wave 0's own work, a miss's new row or a Reserve onto a touched slot,
  // finished before the descriptor is issued.  With KEYS the helper that takes a descriptor also evaluates its row,
  // so a prefetched new slot costs wave 0 one hand-off; waves 1 and 2 take the even and the odd entries, each with
  // its own `handled` counter.  A pod issues at most one descriptor, so kMaxBatch entries suffice.
  //
  // Exactness of two evaluators.  Entries of different slots are independent.  A slot's first descriptor
  // is its creation; every later one comes from a slow pod's Reserve onto the slot, and that Reserve runs after the
  // pod's wait_keys, which covers every descriptor issued so far, the creation and every earlier Reserve included.
  // So the two helpers never write the same skey row concurrently, no helper reads a row while term_take changes it,
  // and when wave 0 has seen both counters reach their shares of its issue count, skey[s][j] is pod j's key on slot s
  // after every pod before j.
  int2* hdesc = reinterpret_cast<int2*>(smem_raw + lay.help);
  int32_t* hpend = reinterpret_cast<int32_t*>(smem_raw + lay.help + (size_t)kMaxBatch * 8);  // descriptors issued
  int32_t* hdone = hpend + 1;                                                                // wave 0 is done
  // {even entries handled by wave 1, odd entries handled by wave 2}: an aligned pair, so wait_keys polls both with
  // one 8-byte LDS read (each half has one writer, which stores its 4 bytes)
  int32_t* heval = hpend + 2;
  uint32_t* skey = reinterpret_cast<uint32_t*>(smem_raw + lay.skey);  // [slot][kSlotKeyStride] (KEYS)
  unsigned long long* hready = reinterpret_cast<unsigned long long*>(smem_raw + lay.help + (size_t)kMaxBatch * 8 + 16);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int32_t cursor0 = __builtin_amdgcn_readfirstlane(*a.cursor);
  if (cursor0 >= a.total_pods) {
    if (threadIdx.x == 0) pipe_next(a, cursor0);  // the queue is done: so are the speculative sweeps after it
    return;
  }
  if (pipe_bubble(a, cursor0)) return;
  const int32_t np = topo_pass_pods(a, cursor0, min(a.batch, a.total_pods - cursor0));
  if (np == 0) return;  // a topology pod at the cursor: the next topology step takes it
#ifdef KS_COMMIT_STAMPS
  // diagnostic build: commit_kernel's stamp points (tools/diag_commit.py), except that the admission is part of the
  // look-ahead's slot 1 and slot 6 is the slow path's wait (KEYS: for both helpers' keys, else for the builder's rows)
  // plus the loop's exit, so slot 2 is the evaluation (KEYS: the key read) and the wave max alone.  The slots mean
  // what they meant when wave 2 alone evaluated.
  uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t tlast = __builtin_amdgcn_s_memtime();
#define KS_FSTAMP(i)                                   \
  do {                                                 \
    const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    ph[i] += t_ - tlast;                               \
    tlast = t_;                                        \
  } while (0)
#else
#define KS_FSTAMP(i) \
  do {               \
  } while (0)
#endif

  for (int64_t c = tid; c < a.nchunks; c += NT) touched[c] = 0ull;
  // lane f < RF_N: the column of row field f (a miss loads its row through it; read with the prologue's loads, so the
  // barrier below does not wait for a round trip of its own)
  const void* my_col = nullptr;
  int32_t my_w = 8;
  if (tid < RF_N) {
    my_col = a.rowcols[lane].p;
    my_w = a.rowcols[lane].width;
  }
  if (a.fq_rec) {
    // ---- the staged prologue: the pass's lists, pods, quota requests and quota table, and the record
    // array the select kernel wrote for the pods at this cursor (FqPassRec: precs, rawtop, rawrun).  Every global
    // load of the prologue is issued before the first LDS store, so the pass arrives in one round trip behind the
    // cursor read: nothing here depends on another load. ----
    constexpr int kRecW = (int)(sizeof(FqPassRec) / 16), kPodW = (int)(sizeof(PodRec) / 16);
    constexpr int kNL = (kMaxBatch * kMaxCand + NT - 1) / NT, kNQ = (kQuotaLdsRows * KS_QUOTA_DIMS + NT - 1) / NT;
    constexpr int kNR = (kQuotaLdsRows + NT - 1) / NT, kNP = (kMaxBatch * KS_QUOTA_DIMS + NT - 1) / NT;
    ProCopy<kNL, NT, uint32_t> c_chunk;
    ProCopy<kNL, NT, uint2> c_t;
    ProCopy<(kMaxBatch * kPodW + NT - 1) / NT, NT, Quad> c_pods;
    ProCopy<(kMaxBatch * kRecW + NT - 1) / NT, NT, Quad> c_rec;
    ProCopy<kNR, NT, int32_t> c_par;
    ProCopy<kNR, NT, uint32_t> c_lm, c_mm;
    ProCopy<kNQ, NT, int64_t> c_lim, c_used, c_min, c_npu;
    const int32_t nl = np * K, nq = a.q.q, nqd = nq * KS_QUOTA_DIMS, nrec = np * kRecW, npq = np * KS_QUOTA_DIMS;
    c_rec.issue(reinterpret_cast<const Quad*>(a.fq_rec), nrec, tid);
    c_chunk.issue(a.cand_chunk, nl, tid);
    c_t.issue(a.cand_t, nl, tid);
    c_pods.issue(reinterpret_cast<const Quad*>(a.pods + cursor0), np * kPodW, tid);
    int64_t rq[kNP];
    // (the request column by selects over opaque scalar copies of the pointers: indexing the kernel argument by dd
    // loads the pointer from memory first, a round trip in front of the request's own)
    const int64_t* qcol[KS_QUOTA_DIMS];
#pragma unroll
    for (int d = 0; d < KS_QUOTA_DIMS; ++d) {
      qcol[d] = a.pq.req[d];
      asm volatile("" : "+s"(qcol[d]));
    }
#pragma unroll
    for (int u = 0; u < kNP; ++u) {
      const int32_t i = tid + u * NT, ii = i < npq ? i : 0;
      const int32_t p = ii / KS_QUOTA_DIMS, dd = ii - p * KS_QUOTA_DIMS;
      const int64_t* col = qcol[0];
#pragma unroll
      for (int d = 1; d < KS_QUOTA_DIMS; ++d) col = dd == d ? qcol[d] : col;
      rq[u] = gld(col + cursor0 + p);  // (a global load: the opaque copies lost their address space)
    }
    c_par.issue(a.q.parent, nq, tid);
    c_lm.issue(a.q.limit_mask, nq, tid);
    c_mm.issue(a.q.min_mask, nq, tid);
    c_lim.issue(a.q.limit, nqd, tid);
    c_used.issue(a.q.used, nqd, tid);
    c_min.issue(a.q.min, nqd, tid);
    c_npu.issue(a.q.npused, nqd, tid);
    asm volatile("" ::: "memory");  // (no load moves below its copy's stores)
#pragma unroll
    for (int u = 0; u < (kMaxBatch * kRecW + NT - 1) / NT; ++u) {
      const int32_t i = tid + u * NT;
      if (i < nrec) {
        const int32_t p = i / kRecW, w = i - p * kRecW;
        Quad* dst = w < 2    ? reinterpret_cast<Quad*>(precs) + p * 2 + w
                     : w < 18 ? reinterpret_cast<Quad*>(rawtop) + p * 16 + (w - 2)
                              : reinterpret_cast<Quad*>(rawrun) + p * 16 + (w - 18);
        *dst = c_rec.v[u];
      }
    }
    c_chunk.store(cand_chunk, nl, tid);
    c_t.store(cand_t, nl, tid);
    c_pods.store(reinterpret_cast<Quad*>(spods), np * kPodW, tid);
#pragma unroll
    for (int u = 0; u < kNP; ++u)
      if (tid + u * NT < npq) pqreq[tid + u * NT] = rq[u];
    c_par.store(qlds->parent, nq, tid);
    c_lm.store(qlds->limit_mask, nq, tid);
    c_mm.store(qlds->min_mask, nq, tid);
    c_lim.store(qlds->limit, nqd, tid);
    c_used.store(qlds->used, nqd, tid);
    c_min.store(qlds->min, nqd, tid);
    c_npu.store(qlds->npused, nqd, tid);
  } else {
    // ---- the gather prologue: the pass's lists and pods, the rows of every pod's top and second-best node from the
    // node columns, the pods' records assembled by wave 0 (passes without a record) ----
    lds_copy<NT>(cand_chunk, a.cand_chunk, np * K, tid);
    lds_copy<NT>(cand_t, a.cand_t, np * K, tid);
    for (int32_t i = tid; i < np * KS_QUOTA_DIMS; i += NT) {
      const int32_t p = i / KS_QUOTA_DIMS, dd = i - p * KS_QUOTA_DIMS;
      pqreq[i] = a.pq.req[dd][cursor0 + p];
    }
    {
      const int64_t* src = reinterpret_cast<const int64_t*>(a.pods + cursor0);
      int64_t* dst = reinterpret_cast<int64_t*>(spods);
      const int32_t words = np * (int32_t)(sizeof(PodRec) / 8);
      lds_copy<NT>(dst, src, words, tid);
    }
    // raw rows of every pod's snapshot-best node (the fast path's winner) and second-best node (the usual winner of a
    // pod whose top an earlier pod took): all loads in flight together
    lds_rawtop<NT>(rawtop, a.cand_top, a.rowcols, np, tid);
    lds_rawtop<NT>(rawrun, a.cand_second, a.rowcols, np, tid);
    for (int32_t r = tid; r < a.q.q; r += NT) {
      qlds->parent[r] = a.q.parent[r];
      qlds->limit_mask[r] = a.q.limit_mask[r];
      qlds->min_mask[r] = a.q.min_mask[r];
    }
    for (int32_t i = tid; i < a.q.q * KS_QUOTA_DIMS; i += NT) {
      qlds->limit[i] = a.q.limit[i];
      qlds->used[i] = a.q.used[i];
      qlds->min[i] = a.q.min[i];
      qlds->npused[i] = a.q.npused[i];
    }
    // wave 0, lane j: pod j's record
    if (tid < 64 && lane < np) {
      const int32_t cnt = a.cand_count[lane];
      const uint64_t second = a.cand_second[lane];
      const uint32_t pmask = a.pq.mask[cursor0 + lane];
      const int32_t quota = a.pods[cursor0 + lane].quota;
      FqPod r;
      r.bound = a.cand_bound[lane];
      r.top = a.cand_top[lane];
      r.flags = a.pods[cursor0 + lane].flags;
      r.qmeta = 0xFFFFu;
      if (quota >= 0) {
        const int32_t pp = a.q.parent[quota];
        r.qmeta = (uint32_t)(pp < 0 ? 0xFFFF : pp) | ((a.q.limit_mask[quota] & 0xFFu) << 16) |
                  ((a.q.min_mask[quota] & 0xFFu) << 24);
      }
      r.qword = (uint32_t)(quota < 0 ? 0xFFFF : quota) | ((pmask & 0xFFu) << 16) | ((uint32_t)max(0, min(cnt, 64)) << 24);
      r.second = (int32_t)gkey_node(second);
      precs[lane] = r;
    }
  }
  if (tid == 0) {
    *hpend = 0;
    *hdone = 0;
    heval[0] = 0;
    heval[1] = 0;
    *hready = 0ull;
  }
  __syncthreads();
  // the other waves are done; wave 0 runs the sequential loop, wave 1 builds slot rows; KEYS: waves 1 and 2 build
  // and evaluate them
  if (tid >= (KEYS ? 192 : 128)) return;
  KS_FSTAMP(0);
  // Opaque copies of the profile words this plugin set reads: hipcc otherwise re-loads kernel-argument words inside
  // the loop (s_load + s_waitcnt lgkmcnt(0)), which would drain every LDS read in flight.  Every other Cfg word is a
  // compile-time zero here (the host routes only such profiles to this kernel).
  Cfg cfg{};
  {
    auto pin = [](int32_t v) {
      asm volatile("" : "+s"(v));
      return v;
    };
    cfg.fit_filter = pin(a.c.fit_filter);
    cfg.fit_score = pin(a.c.fit_score);
    cfg.fw_cpu = pin(a.c.fw_cpu);
    cfg.fw_mem = pin(a.c.fw_mem);
    cfg.fw_eph = pin(a.c.fw_eph);
#pragma unroll
    for (int k = 0; k < NSC; ++k) cfg.fw_sc[k] = pin(a.c.fw_sc[k]);
    cfg.fit_pw = pin(a.c.fit_pw);
    cfg.la_filter = pin(a.c.la_filter);
    cfg.la_score = pin(a.c.la_score);
    cfg.la_prod_usage = pin(a.c.la_prod_usage);
    cfg.lw_cpu = pin(a.c.lw_cpu);
    cfg.lw_mem = pin(a.c.lw_mem);
    cfg.la_pw = pin(a.c.la_pw);
    cfg.quota_enable = 1;
    cfg.quota_parent = pin(a.c.quota_parent);
    cfg.monotone = 1;
  }
  int32_t Kc = K;
  asm volatile("" : "+s"(Kc));

  // ---- per-lane roles in slot construction and Reserve: lane t < kTerms owns slot term t ----
  // capacity / requested raw fields, the PodRec words of its Reserve delta (x1, x100), and whether a zero capacity
  // disables the term (score terms) or not (headrooms)
  constexpr int kTerms = ST_NCPU;  // (the NodeNUMAResource terms of a SlotRow are neither built nor read)
  int32_t t_cap = 0, t_req = 0, t_pw = 0, t_pw100 = 0;
  bool t_prod_only = false, t_score = true;
  switch (lane) {
    case ST_CPU: t_cap = RF_ALLOC_CPU; t_req = RF_NZ_CPU; t_pw = 3; t_pw100 = 12; break;
    case ST_MEM: t_cap = RF_ALLOC_MEM; t_req = RF_NZ_MEM; t_pw = 4; t_pw100 = 13; break;
    case ST_EPH: t_cap = RF_ALLOC_EPH; t_req = RF_REQ_EPH; t_pw = 2; t_pw100 = 14; break;
    case ST_SC + 0: case ST_SC + 1: case ST_SC + 2: case ST_SC + 3:
      t_cap = RF_ALLOC_SC + (lane - ST_SC); t_req = RF_REQ_SC + (lane - ST_SC); t_pw = 7 + (lane - ST_SC); t_pw100 = 17 + (lane - ST_SC);
      break;
    case ST_LCPU: t_cap = RF_LA_ALLOC_CPU; t_req = RF_TERM_CPU; t_pw = 5; t_pw100 = 15; break;
    case ST_LMEM: t_cap = RF_LA_ALLOC_MEM; t_req = RF_TERM_MEM; t_pw = 6; t_pw100 = 16; break;
    case ST_PLCPU: t_cap = RF_LA_ALLOC_CPU; t_req = RF_PTERM_CPU; t_pw = 5; t_pw100 = 15; t_prod_only = true; break;
    case ST_PLMEM: t_cap = RF_LA_ALLOC_MEM; t_req = RF_PTERM_MEM; t_pw = 6; t_pw100 = 16; t_prod_only = true; break;
    case ST_FREE_CPU: t_cap = RF_ALLOC_CPU; t_req = RF_REQ_CPU; t_pw = 0; t_pw100 = 0; t_score = false; break;
    case ST_FREE_MEM: t_cap = RF_ALLOC_MEM; t_req = RF_REQ_MEM; t_pw = 1; t_pw100 = 1; t_score = false; break;
    case ST_FREE_EPH: t_cap = RF_ALLOC_EPH; t_req = RF_REQ_EPH; t_pw = 2; t_pw100 = 2; t_score = false; break;
    case ST_FREE_SC + 0: case ST_FREE_SC + 1: case ST_FREE_SC + 2: case ST_FREE_SC + 3:
      t_cap = RF_ALLOC_SC + (lane - ST_FREE_SC); t_req = RF_REQ_SC + (lane - ST_FREE_SC);
      t_pw = 7 + (lane - ST_FREE_SC); t_pw100 = t_pw; t_score = false; break;
    default: break;
  }
  constexpr int kLaneCounts = ST_N;  // lane: pod count / flags of the row
  // a slot row built from the raw row `src` with pod `podw` already reserved on it (lane-parallel, one code path;
  // every field is read before the first LDS write: the compiler cannot prove the writes do not alias `src`)
  auto build_row = [&](SlotRow* row, const int64_t* src, const int64_t* podw, uint32_t pflags) {
    const bool take = !t_prod_only || (pflags & KS_POD_PROD);
    const int64_t f_cap = src[t_cap], f_req = src[t_req], f_pw = podw[t_pw];
    const int64_t u_bits = src[RF_LA_BITS], u_allowed = src[RF_ALLOWED], u_pods = src[RF_POD_COUNT];
    const int64_t u_acpu = src[RF_ALLOC_CPU], u_amem = src[RF_ALLOC_MEM], u_aeph = src[RF_ALLOC_EPH];
    const int64_t cap = f_cap, req = f_req + (take ? f_pw : 0);
    if (lane < kTerms) {
      Term t;
      t.c = cap;
      t.h = cap - req + ((cap != 0 || !t_score) ? 0 : kNoCap);
      t.hd = cap != 0 ? (double)(cap - req) * 100.0 : 0.0;
      t.r = cap != 0 ? 1.0 / (double)cap : 0.0;
      row->t[lane] = t;
    } else if (lane == kLaneCounts) {
      row->la_bits = (uint32_t)u_bits;
      row->allowed = (int32_t)u_allowed;
      row->pod_count = (int32_t)u_pods + 1;
      row->fit_ws = (u_acpu != 0 ? cfg.fw_cpu : 0) + (u_amem != 0 ? cfg.fw_mem : 0) + (u_aeph != 0 ? cfg.fw_eph : 0);
    }
  };

  if (tid >= 64) {
    // ---- the helper waves, one loop.  Without KEYS wave 1 takes every descriptor and builds its row.  With KEYS
    // wave 1 takes the even entries and wave 2 the odd ones: a helper builds the row of a descriptor without `built`,
    // publishes its ready bit (the write-back and a later Reserve onto the slot wait for it), then evaluates the row
    // for the pods after the issuing one (lane = pod) and bumps its `handled` counter.  For a row it built itself its
    // reads follow its own writes: DS operations of one wave, no cross-wave acquire, so a new slot costs wave 0 one
    // hand-off.  Splitting by entry and not by kind keeps both helpers busy in a run of fast pods, where every
    // descriptor is a build plus an evaluation and wave 0 issues them faster than one wave handles them.
    // Exit: nobody reads the table once wave 0 is done, so after `hdone` a helper skips the evaluations; it still
    // builds every row among its entries (the write-back reads them), and leaves when it has seen `hdone` and then no
    // entry of its own below `hpend` (wave 0 issues nothing after `hdone`). ----
    const int32_t me = KEYS && tid >= 128 ? 1 : 0;
    const PodRec pod = spods[min(lane, np - 1)];  // (KEYS: lane = pod; unused otherwise)
    int32_t next = me, handled = 0;
    for (;;) {
      const int32_t pend =
          __builtin_amdgcn_readfirstlane(__hip_atomic_load(hpend, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (next >= pend) {
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(hdone, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) &&
            next >= __builtin_amdgcn_readfirstlane(__hip_atomic_load(hpend, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)))
          break;
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      const int32_t w = __builtin_amdgcn_readfirstlane(hdesc[next].y);
      // (`hdone` read with the descriptor: a stale 0 only costs an evaluation nobody reads)
      const bool eval =
          KEYS && !__builtin_amdgcn_readfirstlane(__hip_atomic_load(hdone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      const int32_t s = w & 0xFF, jj = (w >> 8) & 0xFF;
      if (!KEYS || !((w >> 17) & 1)) {
        const int64_t* src = (((w >> 16) & 1) ? rawrun : rawtop) + jj * 32;
        const uint32_t pflags = __builtin_amdgcn_readfirstlane(spods[jj].flags);
        build_row(&rows[s], src, reinterpret_cast<const int64_t*>(&spods[jj]), pflags);
        if (lane == 0)
          __hip_atomic_fetch_or(hready, 1ull << s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        // the evaluation below reads what other lanes of this wave wrote: keep the compiler from moving its reads up
        if (KEYS) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
      next += KEYS ? 2 : 1;
      if (eval) {
        NodeReg<NSC> r;
        slot_to_reg<NSC>(rows[s], r);  // wave-uniform address: LDS broadcast reads
        const EvalOut o = eval_pod_node<NSC, false>(cfg, pod, r);
        if (lane > jj && lane < np) skey[s * kSlotKeyStride + lane] = o.reasons == 0 ? (uint32_t)(o.total + 1) : 0u;
        ++handled;
        if (lane == 0) __hip_atomic_store(&heval[me], handled, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    return;
  }
  int32_t hn = 0;     // descriptors issued
  uint64_t hown = 0;  // slots whose rows wave 0 built itself
  // wave 0: every row of `need` is built (the helpers' ready mask or its own)
  auto wait_rows = [&](uint64_t need) {
    if ((hown & need) == need) return;
    for (;;) {
      const uint64_t r =
          readlane64(__hip_atomic_load(hready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP), 0) | hown;
      if ((r & need) == need) break;
      __builtin_amdgcn_s_sleep(1);
    }
  };
  // wave 0 (KEYS): each helper has evaluated its share of the descriptors issued so far, wave 1 the even entries and
  // wave 2 the odd ones (called only inside the pod loop, before `hdone`: both still evaluate what they take)
  auto wait_keys = [&]() {
    for (;;) {
      const uint64_t e = readlane64(
          __hip_atomic_load(reinterpret_cast<unsigned long long*>(heval), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP), 0);
      if ((int32_t)(uint32_t)e >= ((hn + 1) >> 1) && (int32_t)(e >> 32) >= (hn >> 1)) break;
      __builtin_amdgcn_s_sleep(1);
    }
  };
  // wave 0 (KEYS): the descriptor of a row it built or changed itself (the row's LDS writes come first: release).
  // The release store waits for those writes to retire; publishing without that wait would rest on another wave
  // seeing one wave's DS writes in issue order, which the kernel guides do not state, so it stays.
  auto issue_built = [&](int32_t node, int32_t s, int32_t j) {
    if (lane == 0) {
      hdesc[hn] = make_int2(node, s | (j << 8) | (1 << 17));
      __hip_atomic_store(hpend, hn + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    ++hn;
  };

  int32_t snode = -1;  // lane s: node of slot s
  int32_t nslots = 0;
  int32_t processed = np;
  uint32_t rescans = 0, misses = 0, fast = 0;

  // The look-ahead's results for the pod it ran for: its admission status, its record's words (wave-uniform, read
  // from LDS once per pod) and, for a slow pod, its resolved candidates.
  uint32_t st_next = 0, flags_next = 0, qword_next = 0xFFFFu;
  int32_t par_next = -1, second_next = -1;
  uint64_t bound_next = 0;
  int64_t req_next = 0;  // the pod's request in dimension lane & 7 (the admission's read, reused by its usage update)
  Cands cn{};
  auto lookahead = [&](int32_t j) {
    // every LDS read of the record, the admission and the fast check issued together (one latency)
    const uint4 w = *reinterpret_cast<const uint4*>(&precs[j]);
    const ulonglong2 bt = *reinterpret_cast<const ulonglong2*>(&precs[j].bound);
    const uint32_t qm = __builtin_amdgcn_readfirstlane(w.x);
    const uint32_t flags = __builtin_amdgcn_readfirstlane(w.y);
    const uint32_t qw = __builtin_amdgcn_readfirstlane(w.z);
    const bool has_q = (qw & 0xFFFFu) != 0xFFFFu;
    const int32_t qr = has_q ? (int32_t)(qw & 0xFFFFu) : 0;
    const int ld = lane & (KS_QUOTA_DIMS - 1);
    const size_t o = (size_t)qr * KS_QUOTA_DIMS + ld;
    const int64_t req = pqreq[j * KS_QUOTA_DIMS + ld];
    const int64_t u = qlds->used[o], l = qlds->limit[o];
    // the leaf's min check (non-preemptible pods), in the same batch of reads; masks and parent from the record
    const int64_t nu = qlds->npused[o], mn = qlds->min[o];
    const uint64_t top = readlane64(bt.y, 0);
    const int32_t tn = top ? (int32_t)gkey_node(top) : 0;
    const uint64_t tw = touched[tn >> 6];
    const uint32_t lm = (qm >> 16) & 0xFFu, mm = qm >> 24;
    const int32_t par = (qm & 0xFFFFu) == 0xFFFFu ? -1 : (int32_t)(qm & 0xFFFFu);
    req_next = req;
    flags_next = flags;
    qword_next = qw;
    par_next = par;
    second_next = w.w;
    bound_next = bt.x;
    st_next = 0;
    cn.fast = false;
    cn.umax = top;
    if (has_q) {
      // quota_admit's three checks in its order: the leaf's limits, the leaf's min for a non-preemptible pod, the
      // ancestors' limits (the walk up the tree is quota_admit's)
      const uint32_t pmask = (qw >> 16) & 0xFFu;
      const bool in_pod = lane < KS_QUOTA_DIMS && ((pmask >> lane) & 1u);
      if (__ballot(in_pod && ((lm >> lane) & 1u) && (req + u > l))) {
        st_next = KS_S_QUOTA;
      } else if ((flags & KS_POD_NONPREEMPTIBLE) && __ballot(in_pod && ((mm >> lane) & 1u) && (req + nu > mn))) {
        st_next = KS_S_QUOTA_NONPREEMPTIBLE;
      } else if (cfg.quota_parent && par >= 0) {
        st_next = quota_admit(qlds->parent, qlds->limit_mask, qlds->min_mask, qlds->limit, qlds->used, qlds->min,
                              qlds->npused, true, qr, 0u, pmask, req, /*skip_leaf=*/true);
      }
    }
    if (st_next) return;
    if (top && !((tw >> (tn & 63)) & 1ull)) {
      cn.fast = true;  // its row is in rawtop[j]
      return;
    }
    cn = resolve_cands(cand_chunk, cand_t, touched, j, Kc, (int32_t)(qw >> 24));
  };
  lookahead(0);
  KS_FSTAMP(1);

  for (int32_t j = 0; j < np; ++j) {
    const uint32_t st = st_next;
    const Cands cj = cn;
    const int32_t qpar = par_next;
    const int64_t qreq_j = req_next;
    const uint32_t pflags = flags_next, qword = qword_next;
    if (st) {
      if (lane == 0) sres[j] = ks_result{-1, st, 0, -1, 0, 0, 0};
      goto next_pod;
    }
    {
      uint64_t best;
      int32_t node;
      if (cj.fast) {
        // the snapshot-best node is untouched: commits only lower keys, so it wins; no slot holds it, and its row was
        // prefetched at pass start: a helper wave builds the slot
        best = cj.umax;
        ++fast;
        KS_FSTAMP(2);
        node = (int32_t)gkey_node(best);
        const int32_t s = nslots++;
        if (lane == s) snode = node;
        if (lane == 0) {
          atomicOr(&touched[node >> 6], 1ull << (node & 63));
          hdesc[hn] = make_int2(node, s | (j << 8));
          __hip_atomic_store(hpend, hn + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ++hn;
      } else {
        // ---- every touched node exactly (lane = slot), untouched from the candidates ----
        uint64_t key_mod = 0;
        if (KEYS) {
          wait_keys();
          KS_FSTAMP(6);  // (diagnostic builds: the slow path's wait, here for the helpers' keys)
          if (lane < nslots) {
            const uint32_t v = skey[lane * kSlotKeyStride + j];
            if (v) key_mod = ((uint64_t)v << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)snode);  // gkey(v - 1, snode)
          }
        } else {
          wait_rows(nslots >= 64 ? ~0ull : ((1ull << nslots) - 1));
          KS_FSTAMP(6);  // (diagnostic builds: the slow path's wait, here for the builder)
          if (lane < nslots) {
            // pod j: LDS broadcast into VGPRs; flags scalar so the plugin branches stay wave-uniform
            PodRec pod = spods[j];
            pod.flags = pflags;
            NodeReg<NSC> r;
            slot_to_reg<NSC>(rows[lane], r);
            const EvalOut o = eval_pod_node<NSC, false>(cfg, pod, r);
            if (o.reasons == 0) key_mod = gkey(o.total, snode);
          }
        }
        best = umax64(cj.umax, wave_max_u64(key_mod));
        KS_FSTAMP(2);
        uint64_t need = __ballot(!cj.exact && cj.valid && cj.ub > best);
        while (need) {
          // (rescans are rare: the pod's record is read here)
          PodRec pod = spods[j];
          pod.flags = pflags;
          const uint64_t kmax = wave_max_u64(((need >> lane) & 1ull) ? cj.ub : 0ull);
          const int sel = __ffsll((long long)__ballot(((need >> lane) & 1ull) && cj.ub == kmax)) - 1;
          const int64_t c = (int64_t)(uint32_t)__shfl((int)cj.chunk, sel, 64);
          const uint64_t v = fq_rescan<NSC>(a.dn, cfg, pod, c, touched[c], a.n);
          ++rescans;
          best = umax64(best, v);
          need &= ~(1ull << sel);
          need &= __ballot(cj.ub > best);
        }
        if (best < readlane64(bound_next, 0)) {
          processed = j;  // an untouched chunk outside the list may hold a better node: re-sweep from j
          break;
        }
        KS_FSTAMP(3);
        if (best == 0) {
          if (lane == 0) sres[j] = ks_result{-1, KS_S_UNSCHEDULABLE, 0, -1, 0, 0, 0};
          goto next_pod;
        }
        node = (int32_t)gkey_node(best);
        const int64_t* podw = reinterpret_cast<const int64_t*>(&spods[j]);
        // ---- Reserve: NodeInfo.AddPod + podAssignCache.assign on the slot row (lane = term) ----
        int32_t s = __ffsll((long long)__ballot(snode == node)) - 1;
        if (s < 0) {
          // a new slot (never the pod's top node: that one is touched, so a slot holds it)
          s = nslots++;
          if (lane == s) snode = node;
          if (lane == 0) atomicOr(&touched[node >> 6], 1ull << (node & 63));
          if (node == __builtin_amdgcn_readfirstlane(second_next)) {
            // its row was prefetched at pass start: a helper wave builds the slot
            if (lane == 0) {
              hdesc[hn] = make_int2(node, s | (j << 8) | (1 << 16));
              __hip_atomic_store(hpend, hn + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            ++hn;
          } else {
            ++misses;
            if (lane < RF_N) raw[lane] = load_field(my_col, my_w, node);
            hown |= 1ull << s;
            build_row(&rows[s], raw, podw, pflags);
            if (KEYS) issue_built(node, s, j);
          }
        } else {
          wait_rows(1ull << s);
          SlotRow* row = &rows[s];
          const bool take = !t_prod_only || (pflags & KS_POD_PROD);
          if (lane < kTerms) {
            if (take) term_take(row->t[lane], podw[t_pw], __longlong_as_double(podw[t_pw100]));
          } else if (lane == kLaneCounts) {
            row->pod_count += 1;
          }
          if (KEYS) issue_built(node, s, j);
        }
      }
      KS_FSTAMP(4);
      if (lane == 0) sres[j] = ks_result{node, KS_S_SCHEDULED, gkey_score(best), -1, 0, 0, 0};
      if ((qword & 0xFFFFu) != 0xFFFFu) {
        const int32_t qrow = (int32_t)(qword & 0xFFFFu);
        const uint32_t pmask = (qword >> 16) & 0xFFu;
        if (lane < KS_QUOTA_DIMS && ((pmask >> lane) & 1u)) {
          // updatePodUsedNoLock -> updateGroupDeltaUsedNoLock (group_quota_manager.go:620-655): the leaf, then its
          // ancestors.  LDS atomics: no read-back on the sequential path (the next pod's admission reads after them);
          // the request and the leaf's parent are the look-ahead's reads.
          const bool np_ = (pflags & KS_POD_NONPREEMPTIBLE) != 0;
          atomicAdd((unsigned long long*)&qlds->used[(size_t)qrow * KS_QUOTA_DIMS + lane], (unsigned long long)qreq_j);
          if (np_) atomicAdd((unsigned long long*)&qlds->npused[(size_t)qrow * KS_QUOTA_DIMS + lane], (unsigned long long)qreq_j);
          for (int32_t cur = qpar; cur >= 0;) {
            const int32_t up = qlds->parent[cur];
            atomicAdd((unsigned long long*)&qlds->used[(size_t)cur * KS_QUOTA_DIMS + lane], (unsigned long long)qreq_j);
            if (np_) atomicAdd((unsigned long long*)&qlds->npused[(size_t)cur * KS_QUOTA_DIMS + lane], (unsigned long long)qreq_j);
            cur = up;
          }
        }
      }
      KS_FSTAMP(5);
    }
  next_pod:
    if (j + 1 < np) lookahead(j + 1);
    KS_FSTAMP(1);
  }
  KS_FSTAMP(6);
  if (lane == 0) __hip_atomic_store(hdone, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  wait_rows(nslots >= 64 ? ~0ull : ((1ull << nslots) - 1));
  // ---- write back: results, touched rows, quota usage ----
  if (lane < processed) {
    ks_result r = sres[lane];
    topo_writeback(a, cursor0 + lane, r);
    a.results[cursor0 + lane] = r;
  }
  if (lane < nslots) {
    const DevNodes d = *a.dn;
    const SlotRow& r = rows[lane];
    const int64_t node = snode;
    gst(d.req_cpu + node, r.t[ST_FREE_CPU].c - r.t[ST_FREE_CPU].h);
    gst(d.req_mem + node, r.t[ST_FREE_MEM].c - r.t[ST_FREE_MEM].h);
    gst(d.req_eph + node, r.t[ST_FREE_EPH].c - r.t[ST_FREE_EPH].h);
    gst(d.nz_cpu + node, term_requested(r.t[ST_CPU]));
    gst(d.nz_mem + node, term_requested(r.t[ST_MEM]));
#pragma unroll
    for (int k = 0; k < KS_MAX_SCALARS; ++k) gst(d.req_sc[k] + node, r.t[ST_FREE_SC + k].c - r.t[ST_FREE_SC + k].h);
    gst(d.pod_count + node, r.pod_count);
    gst(d.la_term_cpu + node, term_requested(r.t[ST_LCPU]));
    gst(d.la_term_mem + node, term_requested(r.t[ST_LMEM]));
    gst(d.la_pterm_cpu + node, term_requested(r.t[ST_PLCPU]));
    gst(d.la_pterm_mem + node, term_requested(r.t[ST_PLMEM]));
  }
  for (int32_t i = lane; i < a.q.q * KS_QUOTA_DIMS; i += 64) {
    a.q.used[i] = qlds->used[i];
    a.q.npused[i] = qlds->npused[i];
  }
  pipe_carry(a, nslots, snode);
  if (a.top_reset) a.top_reset[lane] = 0ull;
  if (lane == 0) {
    *a.cursor = cursor0 + processed;
    pipe_next(a, cursor0 + processed);
    atomicAdd(&a.counters[0], 1ull);
    if (processed < np) atomicAdd(&a.counters[1], 1ull);
    atomicAdd(&a.counters[2], (unsigned long long)rescans);
    atomicAdd(&a.counters[3], (unsigned long long)misses);
    atomicAdd(&a.counters[15], (unsigned long long)fast);  // ks_stats.diag[7]: monotone fast picks
#ifdef KS_COMMIT_STAMPS
    for (int i = 0; i < 7; ++i) atomicAdd(&a.counters[8 + i], (unsigned long long)ph[i]);
#else
    if (a.fq_rec) atomicAdd(&a.counters[14], 1ull);  // ks_stats.diag[6]: passes loaded by the staged prologue
#endif
  }
#undef KS_FSTAMP
}

// host launch wrappers of the three scalar-slot variants (ks_variant.hip, KS_FEAT == 0)
struct FqLaunch {
  hipError_t (*commit)(bool keys, size_t smem, hipStream_t s, const CommitArgs& a);
  hipError_t (*commit_attr)(bool keys, size_t smem);
};
// (keys: the variant with the slot-key table and the evaluating helper waves; smem includes the table then)
FqLaunch fq_launch_n0();
FqLaunch fq_launch_n2();
FqLaunch fq_launch_n4();

}  // namespace ks
