// Device pieces shared by the grouped MoE expert GEMMs (int4_moe.hip,
// fp8_moe.hip): the per-expert pair list a workgroup builds in LDS from the
// routing, the rows it stands for, and the branch on the row tiles that have
// rows.
//
// A *pair* is p = t * k + j with expert selected[t, j]. Workgroup
// (column block, e) serves the pairs routed to expert e: rows 0 .. count-1
// of its tiles are those pairs, in ascending pair order.
#pragma once

#include "common.h"
#include "dispatch.h"

namespace moe {

constexpr int kWaves = 8;                       // waves of a GEMM workgroup
constexpr int kMaxRows = 64;                    // pairs one expert can take
constexpr int kMaxPairs = kWaves * WAVE_SIZE;   // one routing entry per thread
constexpr int kMaxTopK = 8;
static_assert(kMaxRows * kMaxTopK <= kMaxPairs, "one entry per thread");

// rows 0 .. count-1 of the workgroup's tiles are the listed pairs' rows of y
struct ListedRows {
  const int* list;
  int count;
  DEV_INLINE bool stored(const int r) const { return r < count; }
  DEV_INLINE int row(const int r) const { return list[r]; }
};

// The pairs of `expert`, in ascending pair order: thread p tests entry p
// (n_pairs <= kMaxPairs), a ballot and the waves' counts give its place. The
// list is cut at kMaxRows, so any content of `selected` stays inside it; an
// id outside [0, E) matches no workgroup. Called by all kWaves * WAVE_SIZE
// threads; returns the wave-uniform count. The list is written but not yet
// visible: a workgroup that goes on (count > 0) synchronises before it reads.
DEV_INLINE int build_pair_list(int (&list)[kMaxRows], int (&wave_hits)[kWaves],
                               const int64_t* __restrict__ selected,
                               const int n_pairs, const int expert,
                               const int wave, const int lane) {
  const int p = threadIdx.x;
  const bool hit = p < n_pairs && selected[p] == (int64_t)expert;
  const unsigned long long hits = __ballot(hit);
  if (lane == 0) wave_hits[wave] = __popcll(hits);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = wave_hits[w];
    if (w < wave) before += c;
    total += c;
  }
  const int pos = before + __popcll(hits & ((1ull << lane) - 1ull));
  if (hit && pos < kMaxRows) list[pos] = p;
  return __builtin_amdgcn_readfirstlane(min(total, kMaxRows));
}

// f(Int<LT>) for LT = min(live, MT), live >= 1 and wave-uniform
template <int MT, typename F>
DEV_INLINE void dispatch_live(const int live, F&& f) {
  if constexpr (MT > 1) {
    if (live < MT) return dispatch_live<MT - 1>(live, f);
  }
  f(Int<MT>{});
}

}  // namespace moe
