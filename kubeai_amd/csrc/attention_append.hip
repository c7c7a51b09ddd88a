// Split-KV paged attention for a short chunk of new query rows on top of a
// long cached context ("append": a chat turn after a prefix-cache hit, the
// tail of a chunked prefill, a re-admitted request) for gfx950.
//
// Semantics: kubeai_amd/ops/ref.py::paged_attention_prefill, restricted to
// head_dim 128, no window, no softcap, G in {1,2,4,8}, bf16 or e5m2 cache.
//
// Work split
//  - grid (seq, kv head, q tile x split); a workgroup has G waves, one per q
//    head of the GQA group, and owns ONE 16-row q tile and ONE split of that
//    tile's causal key range [0, ctx + row_lo + n_rows).
//  - a split is a contiguous run of 32-key tiles (two cache blocks) of the
//    tile's own range, ceil(n_tiles / n_splits) each; a surplus split writes
//    (m, l) = (-inf, 0) and returns before it reads the cache.
//  - the q-tile count is sized from Tq on the host (no sync); surplus
//    workgroups exit on query_start_loc.
//  - n_splits == 1 writes bf16 `out` directly. Otherwise every split writes
//    fp32 partials o [S, Tq, n_q, 128], ml [S, Tq, n_q, 2] and
//    append_merge_kernel combines them in increasing split order. No atomics,
//    nothing passes between workgroups: the output is the same bits every run.
//
// Data movement
//  - K tile [32 keys][128] and V tile transposed [128][32 slots] live in one
//    LDS buffer each (16 KB together), staged once per workgroup and read by
//    all G waves: a KV byte crosses HBM once per 16*G query rows and split.
//  - the next tile's global loads are issued into registers before the
//    current tile's MFMAs and land in LDS after them (one buffer, as the
//    decode kernel: a second buffer buys nothing and costs occupancy).
//    A thread stages 8/G consecutive keys of one 8-element head-dim column
//    group, so its transposed V stores pack 4 (G <= 2), 2 (G = 4) or 1
//    (G = 8) keys: 8- / 4- / 2-byte LDS stores.
//  - e5m2 is loaded as raw bytes and converted to bf16 on the way into LDS.
//  - keys at or past the tile's causal limit are staged as zeros, never
//    loaded (their block-table entries may not exist).
//
// Matrix math: v_mfma_f32_16x16x32_bf16, operands swapped relative to
// attention_prefill.hip. Fragment maps of the instruction (q4 = lane >> 4):
//   A[M=16][K=32]: lane holds A[lane & 15][8*q4 + j], j = 0..7
//   B[K=32][N=16]: lane holds B[8*q4 + j][lane & 15]
//   C[M=16][N=16]: lane holds C[4*q4 + i][lane & 15], i = 0..3
//  - scores S^T = K . Q^T, one MFMA chain per 16-key half h of the tile:
//      A = K[16*h + (lane & 15)][32*kc + 8*q4 + j]   (LDS, 16 B read)
//      B = Q[row = lane & 15][32*kc + 8*q4 + j]      (registers, loaded once)
//      C = S^T[key 16*h + 4*q4 + i][row lane & 15]
//    so a lane holds 8 scores of ONE query row, and the row max / sum are
//    2-step reductions over q4 (shfl_xor 16, 32).
//  - output O^T = V^T . P^T. The MFMA's k-slot 8*q4 + j is DEFINED to mean
//    key 4*q4 + (j & 3) + 16*(j >> 2) of the tile (key_slot() is the
//    inverse). With that, the lane's eight probabilities p[h][i], rounded
//    to bf16, ARE its B fragment (j = 4*h + i): P never goes through LDS.
//      B = P^T[slot 8*q4 + j][row lane & 15]         (registers)
//      A = V^T[hd 16*c + (lane & 15)][slot 8*q4 + j] (LDS, 16 B read: V is
//          stored transposed with its keys in slot order)
//      C = O^T[hd 16*c + 4*q4 + i][row lane & 15]
//    so a lane ends with 4 neighbouring head-dim elements of one row per c:
//    one 16 B fp32 partial store or one 8 B bf16 store.
//  - online softmax per row with defer-max: the running max is only raised
//    (and o, l rescaled) when some row of the wave exceeds it by more than 8;
//    l is summed in fp32 from the unrounded p, per lane, and reduced over q4
//    once at the end.
//
// LDS layouts (bytes)
//   K: key*256 + hd*2, 16 B chunk index XOR (key & 7)         (k_off)
//   V: hd*64 + slot*2, 16 B chunk index XOR ((hd>>2)^(hd>>4))&3 (v_off):
//      the 16 rows x 4 chunks one A-fragment read touches are 64 distinct
//      16 B chunks of one 1 KB span, each quarter-wave covering all banks.
#include <torch/extension.h>

#include <type_traits>

#include "attention_checks.h"
#include "attention_plan.h"
#include "common.h"
#include "dispatch.h"

// v_pk_*_f32 stay out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

constexpr int kBS = 16;    // cache block size
constexpr int kQB = 16;    // query rows per tile
constexpr int kKVB = 32;   // keys per tile (2 cache blocks)
constexpr int kHD = 128;   // head dim

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// the types LDS is accessed through: a tile is stored as 16 / 8 / 4 / 2 B
// words and read back as 16 B vectors, so none of them may be assumed
// unrelated to the others
typedef bf16x8 __attribute__((may_alias)) lds_b128;
typedef uint2 __attribute__((may_alias)) lds_b64;
typedef uint32_t __attribute__((may_alias)) lds_b32;
typedef ushort __attribute__((may_alias)) lds_b16;

DEV_INLINE int k_off(const int key, const int hd) {
  return (key * kHD * 2 + hd * 2) ^ ((key & 7) << 4);
}
DEV_INLINE int v_off(const int hd, const int slot) {
  const int sw = ((hd >> 2) ^ (hd >> 4)) & 3;
  return hd * (kKVB * 2) + ((((slot >> 3) ^ sw) << 4) | ((slot & 7) * 2));
}
// MFMA k-slot of tile key t = 16*h + 4*q4 + i: 8*q4 + 4*h + i
DEV_INLINE int key_slot(const int t) {
  return ((t >> 2) & 3) * 8 + (t >> 4) * 4 + (t & 3);
}

template <int G, typename CT>
__launch_bounds__(G * WAVE_SIZE) __global__ void append_attention_kernel(
    ushort* __restrict__ out,            // [Tq, n_q, 128] bf16
    float* __restrict__ part_o,          // [S, Tq, n_q, 128]
    float* __restrict__ part_ml,         // [S, Tq, n_q, 2]
    const ushort* __restrict__ q,        // [Tq, n_q, 128], row stride q_stride
    const CT* __restrict__ k_cache,      // [nb, n_kv, 16, 128]
    const CT* __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,     // [B, max_blocks]
    const int32_t* __restrict__ query_start_loc,  // [B+1]
    const int32_t* __restrict__ seq_lens,         // [B]
    const float scale, const int n_kv, const int max_blocks,
    const int64_t q_stride, const int n_splits,
    const int64_t part_rows) {  // Tq * n_q: rows of one split's partials
  constexpr int NT = G * WAVE_SIZE;
  constexpr int NV = (kKVB * kHD / 8) / NT;  // K (and V) vectors per thread
  constexpr int W = NV >= 4 ? 4 : NV;        // keys packed per V store

  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int qtile = blockIdx.z / n_splits;
  const int split = blockIdx.z % n_splits;
  const int n_q = n_kv * G;
  const int wave = threadIdx.x / WAVE_SIZE;  // = q head within the group
  const int lane = threadIdx.x % WAVE_SIZE;
  const int head = kh * G + wave;
  const int row = lane & 15;  // query row of the tile this lane works for
  const int q4 = lane >> 4;

  const int s0 = query_start_loc[b];
  const int q_len = query_start_loc[b + 1] - s0;
  if (qtile * kQB >= q_len) return;  // whole workgroup exits together
  const int ctx = seq_lens[b] - q_len;  // absolute position of query row 0

  const int row_lo = qtile * kQB;
  const int n_rows = min(kQB, q_len - row_lo);
  const int kv_limit = ctx + row_lo + n_rows;  // causal limit, exclusive
  const int n_tiles = (kv_limit + kKVB - 1) / kKVB;
  const int chunk = (n_tiles + n_splits - 1) / n_splits;
  const int t_lo = split * chunk;
  const int t_hi = min(n_tiles, t_lo + chunk);

  const int64_t tok = s0 + row_lo + row;  // a row of `out` when row < n_rows
  const int64_t prow = (int64_t)split * part_rows + tok * n_q + head;

  if (t_lo >= t_hi) {  // surplus split: nothing of the cache is read
    if (n_splits > 1 && q4 == 0 && row < n_rows) {
      part_ml[prow * 2] = -INFINITY;
      part_ml[prow * 2 + 1] = 0.f;
    }
    return;
  }

  __shared__ __attribute__((aligned(16))) char k_lds[kKVB * kHD * 2];
  __shared__ __attribute__((aligned(16))) char v_lds[kHD * kKVB * 2];

  // ---- Q: the B fragments of the score MFMAs, loaded once ----
  bf16x8 q_frag[kHD / 32];
  {
    const int qrow = min(row_lo + row, q_len - 1);
    const ushort* qp =
        q + (int64_t)(s0 + qrow) * q_stride + (int64_t)head * kHD + q4 * 8;
#pragma unroll
    for (int kc = 0; kc < kHD / 32; ++kc)
      q_frag[kc] = *reinterpret_cast<const bf16x8*>(qp + kc * 32);
  }

  // ---- staging: thread = (8-element column group, NV consecutive keys) ----
  using StageVec = std::conditional_t<sizeof(CT) == 2, bf16x8, uint64_t>;
  StageVec stage_k[NV], stage_v[NV];
  const int col8 = threadIdx.x & 15;
  const int key0 = (threadIdx.x >> 4) * NV;  // first tile key of this thread
  const int32_t* bt = block_tables + (int64_t)b * max_blocks;

  auto issue_tile = [&](const int t) {
    const int abs0 = t * kKVB + key0;  // NV <= 8 keys: all in one cache block
    int64_t blk = 0;
    if (abs0 < kv_limit) blk = bt[min(abs0 / kBS, max_blocks - 1)];
    const int64_t base = ((blk * n_kv + kh) * kBS + abs0 % kBS) * kHD + col8 * 8;
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      if (abs0 + n < kv_limit) {
        stage_k[n] = *reinterpret_cast<const StageVec*>(k_cache + base + n * kHD);
        stage_v[n] = *reinterpret_cast<const StageVec*>(v_cache + base + n * kHD);
      } else {
        // zeros, not stale LDS: p is 0 there, but 0 * NaN would poison o
        stage_k[n] = StageVec{};
        stage_v[n] = StageVec{};
      }
    }
  };
  auto to_bf16 = [](const StageVec& x) {
    if constexpr (sizeof(CT) == 2) {
      return x;
    } else {
      const ushort8 c = e5m2x8_to_bf16x8(x);
      bf16x8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (short)c[j];
      return r;
    }
  };
  auto write_tile = [&]() {
    bf16x8 vv[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      *reinterpret_cast<lds_b128*>(k_lds + k_off(key0 + n, col8 * 8)) =
          to_bf16(stage_k[n]);
      vv[n] = to_bf16(stage_v[n]);
    }
    // V transposed, keys in slot order: W neighbouring keys are W
    // neighbouring slots (key0 + n0 is a multiple of W)
#pragma unroll
    for (int n0 = 0; n0 < NV; n0 += W) {
      const int slot0 = key_slot(key0 + n0);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        char* dst = v_lds + v_off(col8 * 8 + e, slot0);
        if constexpr (W == 4) {
          uint2 pk;
          pk.x = (uint32_t)(ushort)vv[n0][e] |
                 ((uint32_t)(ushort)vv[n0 + 1][e] << 16);
          pk.y = (uint32_t)(ushort)vv[n0 + 2][e] |
                 ((uint32_t)(ushort)vv[n0 + 3][e] << 16);
          *reinterpret_cast<lds_b64*>(dst) = pk;
        } else if constexpr (W == 2) {
          *reinterpret_cast<lds_b32*>(dst) =
              (uint32_t)(ushort)vv[n0][e] |
              ((uint32_t)(ushort)vv[n0 + 1][e] << 16);
        } else {
          *reinterpret_cast<lds_b16*>(dst) = (ushort)vv[n0][e];
        }
      }
    }
  };

  f32x4 o_acc[kHD / 16];
#pragma unroll
  for (int c = 0; c < kHD / 16; ++c) o_acc[c] = {0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY;  // same in the 4 lanes of a row
  float l_run = 0.f;        // this lane's share of the row sum
  const int qpos = ctx + row_lo + row;

  issue_tile(t_lo);
  for (int t = t_lo; t < t_hi; ++t) {
    __syncthreads();  // every wave is done with the previous tile
    write_tile();
    __syncthreads();
    if (t + 1 < t_hi) issue_tile(t + 1);  // in flight under the MFMAs below

    // ---- S^T = K . Q^T, two 16-key halves ----
    f32x4 s_frag[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      s_frag[h] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < kHD / 32; ++kc) {
        const bf16x8 k_frag = *reinterpret_cast<const lds_b128*>(
            k_lds + k_off(h * 16 + row, kc * 32 + q4 * 8));
        s_frag[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag, q_frag[kc], s_frag[h], 0, 0, 0);
      }
    }

    // ---- mask + online softmax: 8 scores of one row per lane ----
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = s_frag[j >> 2][j & 3] * scale;
    const int kv0 = t * kKVB;
    // only tiles that reach past the first row's position need the mask
    // (keys at or past kv_limit are past every row's position)
    if (kv0 + kKVB - 1 > ctx + row_lo) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kpos = kv0 + (j >> 2) * 16 + q4 * 4 + (j & 3);
        if (kpos > qpos) s[j] = -INFINITY;
      }
    }
    float tmax = s[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) tmax = fmaxf(tmax, s[j]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    // defer-max: wave-uniform rescale, only on growth by more than 8
    if (__any(tmax > m_run + 8.f)) {
      const float m_new = fmaxf(m_run, tmax);
      const float corr = (m_new == m_run) ? 1.f : __expf(m_run - m_new);
      l_run *= corr;
#pragma unroll
      for (int c = 0; c < kHD / 16; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) o_acc[c][i] *= corr;
      m_run = m_new;
    }
    bf16x8 p_frag;  // slot 8*q4 + j of P^T, by the definition of the slots
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = (s[j] == -INFINITY) ? 0.f : __expf(s[j] - m_run);
      psum += p;
      p_frag[j] = (short)f32_to_bf16(p);
    }
    l_run += psum;

    // ---- O^T += V^T . P^T ----
#pragma unroll
    for (int c = 0; c < kHD / 16; ++c) {
      const bf16x8 v_frag = *reinterpret_cast<const lds_b128*>(
          v_lds + v_off(c * 16 + row, q4 * 8));
      o_acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v_frag, p_frag,
                                                         o_acc[c], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds hd 16*c + 4*q4 + i of row `row` ----
  float l = l_run;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (row >= n_rows) return;
  if (n_splits == 1) {
    const float inv_l = 1.0f / l;
    ushort* op = out + (tok * n_q + head) * kHD + q4 * 4;
#pragma unroll
    for (int c = 0; c < kHD / 16; ++c) {
      uint2 pk;
      pk.x = (uint32_t)f32_to_bf16(o_acc[c][0] * inv_l) |
             ((uint32_t)f32_to_bf16(o_acc[c][1] * inv_l) << 16);
      pk.y = (uint32_t)f32_to_bf16(o_acc[c][2] * inv_l) |
             ((uint32_t)f32_to_bf16(o_acc[c][3] * inv_l) << 16);
      *reinterpret_cast<uint2*>(op + c * 16) = pk;
    }
  } else {
    // a row with no visible key in this split leaves (-inf, 0) and zeros
    float* po = part_o + prow * kHD + q4 * 4;
#pragma unroll
    for (int c = 0; c < kHD / 16; ++c)
      *reinterpret_cast<f32x4*>(po + c * 16) = o_acc[c];
    if (q4 == 0) {
      part_ml[prow * 2] = m_run;
      part_ml[prow * 2 + 1] = l;
    }
  }
}

// Compile-time split bounds of the merge kernel (append_n_splits caps at 16)
constexpr int kMergeSplitCapLo = 8;
constexpr int kMergeSplitCapHi = 16;
constexpr int kMergeRowsPerBlock = 8;  // 32 lanes x 4 elements per row

// Merge the split partials of one (token, q head) row: 32 lanes, 4 elements
// each. Built as attention_decode.hip's merge_partials: SCAP is a
// compile-time bound on n_splits, every load is issued before any arithmetic
// with the split index clamped to the last real split, an empty (-inf) or
// surplus split is skipped by select (its o was never written), and the sums
// run in increasing split order.
template <int SCAP>
__launch_bounds__(kMergeRowsPerBlock * 32) __global__ void append_merge_kernel(
    ushort* __restrict__ out,           // [Tq, n_q, 128]
    const float* __restrict__ part_o,   // [S, Tq, n_q, 128]
    const float* __restrict__ part_ml,  // [S, Tq, n_q, 2]
    const int n_splits, const int64_t part_rows) {
  const int64_t r =
      (int64_t)blockIdx.x * kMergeRowsPerBlock + threadIdx.x / 32;
  if (r >= part_rows) return;
  const int e0 = (threadIdx.x % 32) * 4;
  floatx2 ml[SCAP];
  f32x4 pv[SCAP];
#pragma unroll
  for (int s = 0; s < SCAP; ++s) {
    const int64_t pr = (int64_t)min(s, n_splits - 1) * part_rows + r;
    ml[s] = *reinterpret_cast<const floatx2*>(part_ml + pr * 2);
    pv[s] = *reinterpret_cast<const f32x4*>(part_o + pr * kHD + e0);
  }
  // keep the scheduler from holding loads back behind the first waits
  __builtin_amdgcn_sched_barrier(0);
  float m_star = -INFINITY;
#pragma unroll
  for (int s = 0; s < SCAP; ++s)
    if (s < n_splits) m_star = fmaxf(m_star, ml[s].x);
  float l_star = 0.f;
  float oo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < SCAP; ++s) {
    const bool use = s < n_splits && ml[s].x != -INFINITY;
    const float c = __expf(ml[s].x - m_star);
    l_star = use ? l_star + ml[s].y * c : l_star;
#pragma unroll
    for (int e = 0; e < 4; ++e) oo[e] = use ? oo[e] + pv[s][e] * c : oo[e];
  }
  const float inv_l = 1.0f / l_star;
  uint2 pk;
  pk.x = (uint32_t)f32_to_bf16(oo[0] * inv_l) |
         ((uint32_t)f32_to_bf16(oo[1] * inv_l) << 16);
  pk.y = (uint32_t)f32_to_bf16(oo[2] * inv_l) |
         ((uint32_t)f32_to_bf16(oo[3] * inv_l) << 16);
  *reinterpret_cast<uint2*>(out + r * kHD + e0) = pk;
}

}  // namespace

#pragma clang attribute pop

// n_splits = 0 takes attn_plan::append_n_splits'. Everything outside the
// kernel's scope is an error raised here, before any launch.
void paged_attention_append(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables,
                            torch::Tensor query_start_loc,
                            torch::Tensor seq_lens, double scale,
                            int64_t n_splits, int64_t window, double softcap) {
  const AttnShape s =
      check_paged_attention(out, q, k_cache, v_cache, block_tables, seq_lens);
  TORCH_CHECK(s.hd == kHD,
              "paged_attention_append supports head_dim 128, not head_dim ",
              s.hd);
  TORCH_CHECK(window == 0 && softcap == 0.0,
              "paged_attention_append supports neither window nor softcap");
  TORCH_CHECK(s.G == 1 || s.G == 2 || s.G == 4 || s.G == 8,
              "paged_attention_append: unsupported GQA group size ", s.G);
  TORCH_CHECK(n_splits >= 0 && n_splits <= kMergeSplitCapHi,
              "paged_attention_append: n_splits must be in [0, 16]");
  const int B = seq_lens.size(0);
  TORCH_CHECK(query_start_loc.scalar_type() == torch::kInt32 &&
              query_start_loc.numel() == B + 1);
  TORCH_CHECK(block_tables.size(0) >= B && s.max_blocks >= 1);
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() &&
              v_cache.scalar_type() == k_cache.scalar_type() &&
              k_cache.size(3) == kHD);
  TORCH_CHECK(out.sizes() == q.sizes());
  // 16 B loads of q and cache rows, 8 B stores of out
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
                  q.stride(0) * q.element_size() % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "paged_attention_append: misaligned q/out/cache");
  const int64_t Tq = q.size(0);
  const int64_t n_qtiles = (Tq + kQB - 1) / kQB;  // per-seq early exit
  if (Tq == 0 || B == 0) return;
  const int S = n_splits > 0 ? (int)n_splits
                             : attn_plan::append_n_splits(Tq, B, s.n_kv,
                                                          s.max_blocks);
  TORCH_CHECK(n_qtiles * S <= 65535 && s.n_kv <= 65535,
              "paged_attention_append: chunk too long for one launch");
  const int64_t part_rows = Tq * s.n_q;
  torch::Tensor part_o, part_ml;
  float *part_o_ptr = nullptr, *part_ml_ptr = nullptr;
  if (S > 1) {
    auto opts = torch::TensorOptions().device(q.device()).dtype(torch::kFloat32);
    part_o = torch::empty({S, Tq, s.n_q, (int64_t)kHD}, opts);
    part_ml = torch::empty({S, Tq, s.n_q, 2}, opts);
    part_o_ptr = part_o.data_ptr<float>();
    part_ml_ptr = part_ml.data_ptr<float>();
  }
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid(B, s.n_kv, (uint32_t)(n_qtiles * S));
  // instantiation set of append_attention_kernel: G {1,2,4,8} x cache type (8)
  dispatch_int<1, 2, 4, 8>(s.G, "GQA group size", [&](auto g) {
    dispatch_bool(s.fp8_cache, [&](auto fp8) {
      constexpr int G = decltype(g)::value;
      using CT = std::conditional_t<decltype(fp8)::value, unsigned char, ushort>;
      hipLaunchKernelGGL(
          (append_attention_kernel<G, CT>), grid, dim3(G * WAVE_SIZE), 0,
          stream, (ushort*)out.data_ptr(), part_o_ptr, part_ml_ptr,
          (const ushort*)q.data_ptr(), (const CT*)k_cache.data_ptr(),
          (const CT*)v_cache.data_ptr(), block_tables.data_ptr<int32_t>(),
          query_start_loc.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
          (float)scale, s.n_kv, s.max_blocks, q.stride(0), S, part_rows);
    });
  });
  HIP_CHECK_KERNEL();
  if (S == 1) return;
  // split-bound tier of the merge kernel
  dispatch_bool(S <= kMergeSplitCapLo, [&](auto lo) {
    constexpr int SCAP =
        decltype(lo)::value ? kMergeSplitCapLo : kMergeSplitCapHi;
    hipLaunchKernelGGL(
        (append_merge_kernel<SCAP>),
        dim3((uint32_t)((part_rows + kMergeRowsPerBlock - 1) /
                        kMergeRowsPerBlock)),
        dim3(kMergeRowsPerBlock * 32), 0, stream, (ushort*)out.data_ptr(),
        part_o_ptr, part_ml_ptr, S, part_rows);
  });
  HIP_CHECK_KERNEL();
}
