// ks_variant.hip — one plugin-set (FEAT = KS_FEAT) x scalar-slot (NSC = KS_NSC) variant of the pass kernels (ks_pass.h) and its host launch
// wrappers.  The Makefile compiles this file once per (FEAT, NSC) so the variants build in parallel, and once more
// with -DKS_NW=8 for the plugin sets with the NUMA topology policy path (FEAT & 8): the kernels at NUMA width 8
// (ks_numa_wide.h).  KS_NW only picks the kernels' NW template argument and the name of the exported table; nothing in
// the headers depends on it, so the objects define no entity twice.
#include "ks_pass.h"
#include "ks_mono.h"
#include "ks_fq.h"

#if !defined(KS_FEAT) || !defined(KS_NSC)
#error "compile with -DKS_FEAT=<feature bits> -DKS_NSC=<0|2|4>"
#endif

#ifndef KS_NW
#define KS_NW 4
#endif
#if KS_NW != 4 && !(KS_NW == 8 && (KS_FEAT & 8) != 0 && KS_FEAT != 31)
#error "KS_NW is 4, or 8 for a plugin set with the NUMA topology policy path (KS_FEAT & 8) other than 31"
#endif

#define KS_CAT2(a, b) a##b
#define KS_CAT(a, b) KS_CAT2(a, b)

namespace ks {
namespace {

constexpr int F = KS_FEAT;

constexpr int NSC = KS_NSC;

constexpr int NW = KS_NW;

hipError_t sweep(int blocks, hipStream_t s, const SweepArgs& a) {
  hipLaunchKernelGGL((sweep_kernel<NSC, F, NW>), dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t commit(bool qc, size_t smem, hipStream_t s, const CommitArgs& a) {
  if (qc) hipLaunchKernelGGL((commit_kernel<NSC, true, F, NW>), dim3(1), dim3(commit_threads(F)), smem, s, a);
  else hipLaunchKernelGGL((commit_kernel<NSC, false, F, NW>), dim3(1), dim3(commit_threads(F)), smem, s, a);
  return hipGetLastError();
}

hipError_t commit_attr(bool qc, size_t smem) {
  const void* fn = qc ? (const void*)commit_kernel<NSC, true, F, NW> : (const void*)commit_kernel<NSC, false, F, NW>;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}

#if (KS_FEAT == 0 || KS_FEAT == 4) && KS_NW == 4
// the plugin sets a nominated table may be loaded with: the NOM variants (ks_nominated.h)
#define KS_HAS_NOM 1
hipError_t sweep_nom(int blocks, hipStream_t s, const SweepArgs& a) {
  hipLaunchKernelGGL((sweep_kernel<NSC, F, NW, true>), dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t commit_nom(bool qc, size_t smem, hipStream_t s, const CommitArgs& a) {
  if (qc) hipLaunchKernelGGL((commit_kernel<NSC, true, F, NW, true>), dim3(1), dim3(commit_threads(F)), smem, s, a);
  else hipLaunchKernelGGL((commit_kernel<NSC, false, F, NW, true>), dim3(1), dim3(commit_threads(F)), smem, s, a);
  return hipGetLastError();
}

hipError_t commit_nom_attr(bool qc, size_t smem) {
  const void* fn = qc ? (const void*)commit_kernel<NSC, true, F, NW, true> : (const void*)commit_kernel<NSC, false, F, NW, true>;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}
#else
constexpr auto sweep_nom = nullptr;
constexpr auto commit_nom = nullptr;
constexpr auto commit_nom_attr = nullptr;
#endif

#if KS_FEAT == 0
// the monotone Fit + LoadAware [+ ElasticQuota] commit (ks_mono.h)
hipError_t commit_mono(bool qc, size_t smem, hipStream_t s, const CommitArgs& a) {
  if (qc) hipLaunchKernelGGL((commit_mono_kernel<NSC, true>), dim3(1), dim3(commit_threads(0)), smem, s, a);
  else hipLaunchKernelGGL((commit_mono_kernel<NSC, false>), dim3(1), dim3(commit_threads(0)), smem, s, a);
  return hipGetLastError();
}

hipError_t commit_mono_attr(bool qc, size_t smem) {
  const void* fn = qc ? (const void*)commit_mono_kernel<NSC, true> : (const void*)commit_mono_kernel<NSC, false>;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}

// the monotone Fit + LoadAware + ElasticQuota commit with the quota tables in LDS (ks_fq.h)
hipError_t commit_fq(bool keys, size_t smem, hipStream_t s, const CommitArgs& a) {
  if (keys) hipLaunchKernelGGL((commit_fq_kernel<NSC, true>), dim3(1), dim3(commit_threads(0)), smem, s, a);
  else hipLaunchKernelGGL((commit_fq_kernel<NSC, false>), dim3(1), dim3(commit_threads(0)), smem, s, a);
  return hipGetLastError();
}

hipError_t commit_fq_attr(bool keys, size_t smem) {
  const void* fn = keys ? (const void*)commit_fq_kernel<NSC, true> : (const void*)commit_fq_kernel<NSC, false>;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}
#endif

#if (KS_FEAT & 8) != 0
hipError_t reserve_pre(int blocks, hipStream_t s, const CommitArgs& a) {
  hipLaunchKernelGGL((reserve_pre_kernel<F, NW>), dim3(blocks), dim3(64), 0, s, a);
  return hipGetLastError();
}
#endif

}  // namespace

#if KS_NW == 8
PassLaunch KS_CAT(KS_CAT(KS_CAT(KS_CAT(pass_launch_f, KS_FEAT), _n), KS_NSC), _w8)() {
#else
PassLaunch KS_CAT(KS_CAT(KS_CAT(pass_launch_f, KS_FEAT), _n), KS_NSC)() {
#endif
#if KS_FEAT == 0
  return PassLaunch{sweep, commit, commit_attr, commit_mono, commit_mono_attr, nullptr, sweep_nom, commit_nom, commit_nom_attr};
#elif (KS_FEAT & 8) != 0
  return PassLaunch{sweep, commit, commit_attr, nullptr, nullptr, reserve_pre, sweep_nom, commit_nom, commit_nom_attr};
#else
  return PassLaunch{sweep, commit, commit_attr, nullptr, nullptr, nullptr, sweep_nom, commit_nom, commit_nom_attr};
#endif
}

#if KS_FEAT == 0
FqLaunch KS_CAT(fq_launch_n, KS_NSC)() { return FqLaunch{commit_fq, commit_fq_attr}; }
#endif

}  // namespace ks
