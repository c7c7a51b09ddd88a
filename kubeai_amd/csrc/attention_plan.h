// Host-side launch plans of the attention kernels: which prefill kernel a
// shape runs (v1 / v2, workgroup width) and how many flash-decoding splits
// a decode batch gets. Pure functions of the shape plus the tuning env
// overrides — the launchers call them, and bindings.cpp exposes them
// (_C.prefill_plan / _C.decode_plan) so a test can assert the path a case
// was written for instead of trusting a comment.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace attn_plan {

constexpr int kBlockSize = 16;  // cache block size (tokens)

// ---- env overrides (read once per process) ----------------------------
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// KUBEAI_PREFILL_V2=0 sends every prefill to v1
inline bool env_use_v2() {
  static const bool v = []() {
    const char* e = getenv("KUBEAI_PREFILL_V2");
    return e == nullptr || e[0] != '0';
  }();
  return v;
}
// KUBEAI_V2_WAVES=4|8 forces the v2 workgroup width (G <= 4)
inline int env_v2_waves() {
  static const int v = env_int("KUBEAI_V2_WAVES", 0);
  return v;
}
// KUBEAI_V2_DBG: compile-time bisect switches of the v2 kernel
inline int env_v2_dbg() {
  static const int v = env_int("KUBEAI_V2_DBG", 0);
  return v;
}
// KUBEAI_V2_OCC=4: the 4-waves/SIMD launch-bounds experiment
inline int env_v2_occ() {
  static const int v = env_int("KUBEAI_V2_OCC", 2);
  return v;
}
inline int env_decode_split_target() {
  static const int v = []() {
    const int t = env_int("KUBEAI_DECODE_SPLIT_TARGET", 2048);
    return t > 0 ? t : 2048;
  }();
  return v;
}
inline int env_decode_min_blocks_per_split() {
  static const int v = env_int("KUBEAI_DECODE_MIN_BLOCKS_PER_SPLIT", 0);
  return v;
}

// ---- prefill ------------------------------------------------------------
struct PrefillPlan {
  int version;  // 1 = attention_prefill.hip, 2 = attention_prefill_v2.hip
  int waves;    // waves per workgroup (v1: one per q head of the group)
};

// v2 workgroup width, or 0 when v2 does not take the shape (v1 runs).
inline int prefill_v2_waves(int64_t Tq, int B, int n_q, int n_kv, int hd,
                            int max_blocks) {
  const int G = n_q / n_kv;
  if (hd != 128 || (G != 1 && G != 2 && G != 4 && G != 8)) return 0;
  // small-q chunked continuations underfill the 8-wave workgroups
  // (few z-tiles); v1's 16-row tiles win there (profiles/r02)
  if (Tq <= 1024 && B == 1) {
    // rough ctx estimate via block-table width (host-side, no sync)
    const int64_t approx_L = (int64_t)max_blocks * kBlockSize;
    if (approx_L > 3 * Tq) return 0;
  }
  // workgroup width: 8 waves (256 q rows/WG, best arithmetic intensity)
  // unless that would underfill the 256-CU chip — small prefills then
  // run the 4-wave form, whose 2x workgroup count fills more CUs
  // (measured: +11% at Tq=1024, -6% at Tq=8192 — same-box A/B).
  // KUBEAI_V2_WAVES forces either.
  int nw = 8;
  // the DBG and OCC=4 experiment kernels exist in the 8-wave form only
  const bool only8 = (env_v2_dbg() & 3) != 0 || env_v2_occ() == 4;
  if (G <= 4 && !only8) {
    const int forced = env_v2_waves();
    if (forced == 4 || forced == 8) {
      nw = forced;
    } else {
      const int qrows8 = (8 / G) * 32;
      const int64_t wgs8 = (int64_t)B * n_kv * ((Tq + qrows8 - 1) / qrows8);
      if (wgs8 < 256) nw = 4;
    }
  }
  return nw;
}

inline PrefillPlan prefill_plan(int64_t Tq, int B, int n_q, int n_kv, int hd,
                                int max_blocks, int64_t window,
                                double softcap) {
  // the v2 ladder covers the plain-causal hd=128 fast path only (its
  // interior-tile fast path has no sliding-window masking)
  if (window == 0 && softcap == 0.0 && env_use_v2()) {
    const int nw = prefill_v2_waves(Tq, B, n_q, n_kv, hd, max_blocks);
    if (nw) return {2, nw};
  }
  return {1, n_q / n_kv};
}

// ---- decode ---------------------------------------------------------------
// flash-decoding split: target 2048 workgroups, cap 16. Fixed-shape
// microbenches (scripts/sweep_decode_splits.py) mildly favor 4096, but
// the live bench's length mix loses ~4.5% end-to-end at 4096 (extra
// fp32 partial traffic + merge work inside graph replay) — same-box
// A/B in profiles/r01_results.md. KUBEAI_DECODE_SPLIT_TARGET overrides
// for tuning sweeps. KUBEAI_DECODE_MIN_BLOCKS_PER_SPLIT is the optional
// length-aware bound: >=N cache blocks per split, so short sequences
// don't launch mostly-empty splits (max_blocks is the widest block table
// this step — host-side, no device sync).
inline int decode_n_splits(int B, int n_kv, int max_blocks) {
  const int split_target = env_decode_split_target();
  const int min_blocks_per_split = env_decode_min_blocks_per_split();
  int n_splits = 1;
  const int base_wgs = B * n_kv;
  if (base_wgs > 0 && base_wgs < split_target) {
    n_splits = std::min<int>(16, (split_target + base_wgs - 1) / base_wgs);
    if (min_blocks_per_split > 0) {
      const int cap = std::max(1, max_blocks / min_blocks_per_split);
      n_splits = std::min(n_splits, cap);
    }
  }
  return n_splits;
}

}  // namespace attn_plan
