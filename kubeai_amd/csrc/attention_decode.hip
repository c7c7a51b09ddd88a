// Paged-attention decode (one new token per sequence) for gfx950.
//
// Semantics: kubeai_amd/ops/ref.py::paged_attention_decode.
//
// Design (MI355X-first, memory-bound regime — see guide Appendix B):
//  - workgroup = (seq, kv_head); 4 waves; GQA group of G = n_q/n_kv query
//    heads computed together so each KV byte is read from HBM exactly once.
//  - waves process DISJOINT cache blocks (flash-decoding split): wave w takes
//    blocks w, w+4, ... with per-wave online-softmax state, merged at the end
//    through LDS (m*, l*, o* combine). This keeps the chip busy at small
//    decode batches (B*n_kv*4 waves in flight).
//  - each wave stages its 16-token KV tile into its own LDS buffer with
//    ushort8 (16 B) vector loads (rows padded 16 B for bank spread).
//  - scoring is token-parallel: 4 lanes per token, each covering a 32-elem
//    head_dim slice, 2-step part reduction — one pass scores the whole tile
//    (v1's 16 serial 64-lane butterflies were the VALU bottleneck).
//  - tile-level online softmax with defer-max (rescale only when the
//    running max grows); PV accumulates per-lane head_dim pairs with the
//    per-token p reaching lanes via one __shfl broadcast.
#include <torch/extension.h>

#include <type_traits>

#include "attention_checks.h"
#include "attention_plan.h"
#include "common.h"
#include "dispatch.h"

namespace {

// 2 waves/workgroup, one LDS tile buffer each: 21.5 KB at G = 4, hd 128,
// bf16, which lets 6 workgroups share a CU (profiles/r09_decode_step.md)
constexpr int kWaves = 2;
constexpr int kBlockThreads = kWaves * WAVE_SIZE;
constexpr int kBS = 16;   // cache block size (tokens)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;  // v_dot2 operand
// +8 ushorts (16 B) row padding: keeps 16 B staging alignment and breaks
// the power-of-two row stride so the (token, part) score reads spread
// over banks (4-way residual aliasing ~= 1.6x on the LDS op, vs 32-way
// unpadded)
constexpr int kPad = 8;

// CT = cache element type: ushort (bf16) or unsigned char (fp8 e5m2,
// converted to bf16 in-register while staging — same LDS layout/compute)
// HD = head dim: 128 (llama family) or 256 (gemma2). A lane always
// covers a 32-element slice, so HD sets PARTS = HD/32 lanes per token
// and TOKP = 64/PARTS tokens scored per pass (two passes per 16-token
// tile at HD=256).
// SOFTCAP > 0 applies gemma2-style attention-logit soft capping,
// s = cap * tanh(s / cap), after scaling and before masking.
// CAP: compile-time softcap enable — a runtime branch in the score
// loop measured -13% on the capless hot path (194.6 vs 169.0 us at
// B=64 L=2048), so capped models get their own instantiation.
//
// RAW: "raw qkv" mode of a pure-decode step (rope_cache_attention_decode).
// q is the UNROTATED projection output and k_new / v_new hold the new
// token's raw K/V heads. The kernel rotates q on the way into q_pack, and
// the one wave that owns cache block (L-1)/16 rotates k, stores the new K/V
// row into the cache at slot_mapping[b] and patches the same bytes into its
// own LDS tile, so the row never has to come back through memory. Equals
// rope_and_cache followed by the !RAW kernel bit for bit in out and in both
// caches; q, k_new and v_new are only read.
template <int G, typename CT = ushort, int HD = 128, bool CAP = false,
          bool RAW = false>
__launch_bounds__(kBlockThreads) __global__ void paged_decode_kernel(
    ushort* __restrict__ out,            // [B, n_q, hd] bf16
    const ushort* __restrict__ q,        // [B, n_q, hd] bf16
    // [nb, n_kv, bs, hd]; written (one row per (b, kv head)) only when RAW
    std::conditional_t<RAW, CT*, const CT*> __restrict__ k_cache,
    std::conditional_t<RAW, CT*, const CT*> __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,  // [B, max_blocks]
    const int32_t* __restrict__ seq_lens,      // [B]
    const float scale, const float softcap, const int window,
    const int n_kv, const int max_blocks,
    const int64_t q_stride, const int n_splits,
    float* __restrict__ part_o,    // [B, n_q, n_splits, hd]
    float* __restrict__ part_ml,   // [B, n_q, n_splits, 2]
    // RAW only (null / 0 otherwise)
    const ushort* __restrict__ k_new,          // [B, n_kv, hd] bf16, unrotated
    const ushort* __restrict__ v_new,          // [B, n_kv, hd] bf16
    const int32_t* __restrict__ positions,     // [B]
    const float* __restrict__ cos_sin,         // [max_pos, hd]
    const int64_t* __restrict__ slot_mapping,  // [B]
    const int64_t k_stride, const int64_t v_stride) {
  const int b = blockIdx.x / (n_kv * n_splits);
  const int rem = blockIdx.x % (n_kv * n_splits);
  const int kh = rem / n_splits;
  const int split = rem % n_splits;
  const int n_q = n_kv * G;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int L = seq_lens[b];
  // RAW: the row's position and slot are read next to seq_lens so that the
  // three scalar loads share one round trip (read where they are used, each
  // cost a trip of its own: the compiler waits on a scalar load at once)
  int pos = 0;
  int64_t slot = -1;
  if constexpr (RAW) {
    pos = positions[b];
    slot = slot_mapping[b];
  }
  const int n_blocks = (L + kBS - 1) / kBS;
  // sliding window: the query (position L-1) attends keys in
  // (L-1-window, L-1] -> global positions >= w0; whole blocks below w0
  // are skipped, the straddling block is masked per token
  const int w0 = (window > 0) ? max(0, L - window) : 0;
  // flash-decoding splits divide the WINDOWED block range — splitting
  // the full range would leave every split below w0 empty for long
  // sequences (mistral at L >> window would use a fraction of the
  // launched workgroups)
  const int blk_base = w0 / kBS;
  const int n_eff = n_blocks - blk_base;
  const int chunk = (n_eff + n_splits - 1) / n_splits;
  const int blk_lo = blk_base + split * chunk;
  const int blk_hi = min(n_blocks, blk_lo + chunk);

  // LDS: one KV tile buffer per wave + merge scratch. The wave that reads a
  // tile is the wave that overwrites it with the next one, after the compute,
  // in program order (LDS operations of one wave complete in order), so a
  // second buffer would buy nothing and cost occupancy. Element type
  // follows the cache: bf16 stages bf16; fp8 stages the RAW e5m2 bytes
  // (half the LDS footprint/traffic) and converts during compute with the
  // native packed bf8->f32 instruction (v_cvt_pk_f32_bf8). 8-element row
  // pad keeps 8 B staging alignment and breaks bank aliasing for both
  // element widths (bf16: 68-dword stride, gcd 4; fp8: 34-dword, gcd 2).
  constexpr int PARTS = HD / 32;    // lanes per token in scoring
  constexpr int TOKP = 64 / PARTS;  // tokens scored per pass
  constexpr int EPL = HD / 64;      // output elems owned per lane
  __shared__ CT k_lds[kWaves][kBS][HD + kPad];
  __shared__ CT v_lds[kWaves][kBS][HD + kPad];
  __shared__ float merge_o[kWaves][G][HD];
  __shared__ float merge_ml[kWaves][G][2];

  // --- lane roles -----------------------------------------------------
  // scoring: PARTS lanes per token, each covering a 32-elem slice of
  //   head_dim — TOKP tile tokens score in parallel with a log2(PARTS)-
  //   step part reduction (replaces v1's serial 64-lane butterflies)
  // PV/output: lane owns head_dim elems [EPL*lane, EPL*lane+EPL);
  //   per-token p reaches every lane via one __shfl broadcast
  const int tok_of = lane / PARTS;
  const int part = lane % PARTS;

  // q slice for this lane's part, packed bf16 pairs (16 u32 per head)
  uint32_t q_pack[G][16];
  if constexpr (!RAW) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t* qp = reinterpret_cast<const uint32_t*>(
          q + (int64_t)b * q_stride + (int64_t)(kh * G + g) * HD + part * 32);
#pragma unroll
      for (int i = 0; i < 16; ++i) q_pack[g][i] = qp[i];
    }
  }

  // RAW: the block-table entry of this wave's first tile is asked for ahead
  // of the prologue loads, so the tile loads can go out as soon as it is
  // back (index clamped to a valid entry when the wave has no tile)
  const int32_t* bt = block_tables + (int64_t)b * max_blocks;
  const int first = blk_lo + wave;
  int64_t blk_first = 0;
  if constexpr (RAW) blk_first = bt[first < blk_hi ? first : 0];

  // ---- RAW prologue, loads only: nothing here depends on seq_lens, so
  // these are in flight while the seq_lens -> block table -> KV tile chain
  // resolves (the cos_sin row sits at the depth of the block-table load)
  constexpr int HALF = HD / 2;
  // q: the group's G*HALF rotary pairs are spread over the wave, 4 pairs
  // per lane and pass (8 B loads), instead of every lane rotating its own
  // 32-element slice of every head (16x redundant across the token lanes)
  constexpr int QV = G * HALF / 4;                        // 4-pair vectors
  constexpr int QIT = (QV + WAVE_SIZE - 1) / WAVE_SIZE;   // passes
  ushort4_t q_lo[RAW ? QIT : 1], q_hi[RAW ? QIT : 1];
  float4_t q_c[RAW ? QIT : 1], q_s[RAW ? QIT : 1];
  // new K/V row: lanes [0, HD/8) take one 8-element vector of k each,
  // lanes [HD/8, HD/4) one of v
  constexpr int RV = HD / 8;
  ushort8 row_own, row_par;
  float4_t row_c[2], row_s[2];
  const bool row_hi = (lane % RV) >= RV / 2;  // vector in the second half
  if constexpr (RAW) {
    const float* cs = cos_sin + (int64_t)pos * HD;
#pragma unroll
    for (int it = 0; it < QIT; ++it) {
      const int idx = lane + it * WAVE_SIZE;
      if (QV % WAVE_SIZE == 0 || idx < QV) {
        const int g = idx / (HALF / 4);
        const int i = (idx % (HALF / 4)) * 4;
        const ushort* qh =
            q + (int64_t)b * q_stride + (int64_t)(kh * G + g) * HD + i;
        q_lo[it] = *reinterpret_cast<const ushort4_t*>(qh);
        q_hi[it] = *reinterpret_cast<const ushort4_t*>(qh + HALF);
        q_c[it] = *reinterpret_cast<const float4_t*>(cs + i);
        q_s[it] = *reinterpret_cast<const float4_t*>(cs + HALF + i);
      }
    }
    // every lane loads (lanes past 2 * RV repeat the first ones, v lanes
    // load a partner and angles they do not use): no branch here, so no
    // wait ahead of the block-table load
    {
      const int e0 = (lane % RV) * 8;
      const ushort* row = ((lane / RV) % 2 == 0
                               ? k_new + (int64_t)b * k_stride
                               : v_new + (int64_t)b * v_stride) +
                          (int64_t)kh * HD;
      row_own = *reinterpret_cast<const ushort8*>(row + e0);
      row_par = *reinterpret_cast<const ushort8*>(
          row + (row_hi ? e0 - HALF : e0 + HALF));
      const int i = row_hi ? e0 - HALF : e0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        row_c[h] = *reinterpret_cast<const float4_t*>(cs + i + 4 * h);
        row_s[h] = *reinterpret_cast<const float4_t*>(cs + HALF + i + 4 * h);
      }
    }
  }

  float m[G], l[G], o[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }

  // T14 async-stage: global loads for block n+1 issue before block n's
  // compute (their latency hides under it); the register payload lands in
  // the wave's LDS buffer once block n's compute has read it. Per-wave
  // buffers -> no barriers anywhere in the loop.
  // staging vector = 8 elements: 16 B (bf16) or 8 B (raw fp8 bytes)
  using StageVec = std::conditional_t<sizeof(CT) == 2, ushort8, uint64_t>;
  constexpr int NS = (kBS * HD / 8) / WAVE_SIZE;
  StageVec stage_k[NS], stage_v[NS];  // this lane's vectors of each tile
  // The type LDS is written through. A tile is stored as staging vectors and
  // read back as 4- and 2-byte words; the fp8 vector is a plain uint64_t,
  // which type-based alias analysis takes to be unrelated to those reads.
  // With the one buffer at a fixed address the compiler then moved the first
  // tile's reads above its stores. may_alias keeps program order (the bf16
  // vector type aliases everything already).
  typedef StageVec __attribute__((may_alias)) LdsVec;

  auto issue_tile = [&](const int64_t blk) {
    const CT* base_k = k_cache + ((blk * n_kv + kh) * kBS) * HD;
    const CT* base_v = v_cache + ((blk * n_kv + kh) * kBS) * HD;
    const StageVec* src_k = reinterpret_cast<const StageVec*>(base_k);
    const StageVec* src_v = reinterpret_cast<const StageVec*>(base_v);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      stage_k[i] = src_k[lane + i * WAVE_SIZE];
      stage_v[i] = src_v[lane + i * WAVE_SIZE];
    }
  };
  auto issue_loads = [&](int blk_i) { issue_tile(bt[blk_i]); };
  auto write_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int vec = lane + i * WAVE_SIZE;  // 8-element vector index
      const int row = vec / (HD / 8);
      const int col = vec % (HD / 8);
      *reinterpret_cast<LdsVec*>(&k_lds[wave][row][col * 8]) = stage_k[i];
      *reinterpret_cast<LdsVec*>(&v_lds[wave][row][col * 8]) = stage_v[i];
    }
  };

  if (first < blk_hi) {
    if constexpr (RAW)
      issue_tile(blk_first);
    else
      issue_loads(first);
  }

  // the new row's cache block and the bytes this lane patches into its
  // LDS tile; row_blk stays -1 in every wave but the owner
  int row_blk = -1;
  StageVec row_vec{};
  if constexpr (RAW) {
    // rotate q through the merge scratch of this wave (idle until the
    // epilogue, private to the wave until the barrier there): bf16 [G][HD]
    ushort* q_rot = reinterpret_cast<ushort*>(&merge_o[wave][0][0]);
#pragma unroll
    for (int it = 0; it < QIT; ++it) {
      const int idx = lane + it * WAVE_SIZE;
      if (QV % WAVE_SIZE == 0 || idx < QV) {
        const int g = idx / (HALF / 4);
        const int i = (idx % (HALF / 4)) * 4;
        ushort4_t r_lo, r_hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ushort o1, o2;
          rope_rotate_pair(bf16_to_f32(q_lo[it][e]), bf16_to_f32(q_hi[it][e]),
                           q_c[it][e], q_s[it][e], o1, o2);
          r_lo[e] = o1;
          r_hi[e] = o2;
        }
        *reinterpret_cast<ushort4_t*>(q_rot + g * HD + i) = r_lo;
        *reinterpret_cast<ushort4_t*>(q_rot + g * HD + HALF + i) = r_hi;
      }
    }
    // same wave wrote and reads: LDS ops of a wave complete in order
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint4* qp =
          reinterpret_cast<const uint4*>(q_rot + g * HD + part * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint4 t = qp[i];
        q_pack[g][4 * i] = t.x;
        q_pack[g][4 * i + 1] = t.y;
        q_pack[g][4 * i + 2] = t.z;
        q_pack[g][4 * i + 3] = t.w;
      }
    }

    // new K/V row: exactly one wave per (b, kv head) owns cache block
    // (L-1)/16 — the split whose block range holds it, and in that split
    // the wave whose stride lands on it. slot < 0 (graph pad row): nothing
    // is stored or patched, the row attends what the cache already holds.
    const int new_blk = (L - 1) / kBS;
    const bool owner = slot >= 0 && L > 0 && new_blk >= blk_lo &&
                       new_blk < blk_hi && (new_blk - blk_lo) % kWaves == wave;
    if (owner) {
      row_blk = new_blk;
      if (lane < 2 * RV) {
        ushort8 row = row_own;  // v: stored as it is
        if (lane < RV) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x_own = bf16_to_f32(row_own[e]);
            const float x_par = bf16_to_f32(row_par[e]);
            ushort o1, o2;
            rope_rotate_pair(row_hi ? x_par : x_own, row_hi ? x_own : x_par,
                             row_c[e / 4][e % 4], row_s[e / 4][e % 4], o1, o2);
            row[e] = row_hi ? o2 : o1;
          }
        }
        if constexpr (sizeof(CT) == 2) {
          row_vec = row;
        } else {
          // bf16x8_to_e5m2x8, spelled out: through the helper the compiler
          // schedules these kernels differently
          // (profiles/r06_launch_dispatch.md)
          row_vec = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            row_vec |= (uint64_t)f32_to_e5m2(bf16_to_f32((ushort)row[e]))
                       << (8 * e);
        }
        CT* dst = (lane < RV ? k_cache : v_cache) +
                  cache_row_offset(slot, kBS, n_kv, kh, HD) + (lane % RV) * 8;
        *reinterpret_cast<StageVec*>(dst) = row_vec;
      }
    }
  }
  if (first < blk_hi) write_tile();

  for (int blk_i = first; blk_i < blk_hi; blk_i += kWaves) {
    const int tile_start = blk_i * kBS;
    const int tile_len = min(kBS, L - tile_start);
    if (blk_i + kWaves < blk_hi) issue_loads(blk_i + kWaves);

    if constexpr (RAW) {
      // the tile of the new row's block was staged from memory without
      // that row: put the bytes just stored over it (same wave as the
      // write_tile before, program order — no barrier)
      if (blk_i == row_blk && lane < 2 * RV) {
        CT* dst = lane < RV ? &k_lds[wave][(L - 1) % kBS][lane * 8]
                            : &v_lds[wave][(L - 1) % kBS][(lane - RV) * 8];
        *reinterpret_cast<LdsVec*>(dst) = row_vec;
      }
    }

    // TOKP tokens score per pass; kBS/TOKP passes cover the tile (one
    // pass at HD=128, two at HD=256)
#pragma unroll
    for (int tp = 0; tp < kBS; tp += TOKP) {
      const int tok = tp + tok_of;
      // ---- scores: lane computes its (token, part-slice) partial ------
      float s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = 0.f;
      if constexpr (sizeof(CT) == 2) {
        // v_dot2c_f32_bf16: one instruction per bf16 pair-dot-accumulate
        // (replaces 2 unpacks + 2 fma per (g, j) — a 3x VALU cut in the
        // score phase)
        const uint32_t* krow = reinterpret_cast<const uint32_t*>(
            &k_lds[wave][tok][part * 32]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const bf16x2v kk = __builtin_bit_cast(bf16x2v, krow[j]);
#pragma unroll
          for (int g = 0; g < G; ++g)
            s[g] = __builtin_amdgcn_fdot2_f32_bf16(
                kk, __builtin_bit_cast(bf16x2v, q_pack[g][j]), s[g], false);
        }
      } else {
        // raw e5m2 slice: each uint32 holds 4 bytes -> 4 elements; the
        // packed bf8->f32 convert does 2 per instruction
        const uint32_t* krow = reinterpret_cast<const uint32_t*>(
            &k_lds[wave][tok][part * 32]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t kk = krow[j];
          const floatx2 k01 = __builtin_amdgcn_cvt_pk_f32_bf8(kk, false);
          const floatx2 k23 = __builtin_amdgcn_cvt_pk_f32_bf8(kk, true);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const uint32_t qa = q_pack[g][2 * j];
            const uint32_t qb = q_pack[g][2 * j + 1];
            s[g] = fmaf(k01.x, bf16_to_f32((ushort)(qa & 0xffff)), s[g]);
            s[g] = fmaf(k01.y, bf16_to_f32((ushort)(qa >> 16)), s[g]);
            s[g] = fmaf(k23.x, bf16_to_f32((ushort)(qb & 0xffff)), s[g]);
            s[g] = fmaf(k23.y, bf16_to_f32((ushort)(qb >> 16)), s[g]);
          }
        }
      }
      float p[G];
      float rsum[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        // reduce across the part-slices -> full dot in all PARTS lanes
#pragma unroll
        for (int off = 1; off < PARTS; off <<= 1)
          s[g] += __shfl_xor(s[g], off, 64);
        s[g] = (tok < tile_len && tile_start + tok >= w0) ? s[g] * scale
                                                          : -INFINITY;
        if constexpr (CAP) {
          if (s[g] != -INFINITY) s[g] = softcap * tanhf(s[g] / softcap);
        }
        // pass max across tokens (lane bits above the part bits)
        float tmax = s[g];
#pragma unroll
        for (int off = PARTS; off < 64; off <<= 1)
          tmax = fmaxf(tmax, __shfl_xor(tmax, off, 64));
        const float m_new = fmaxf(m[g], tmax);
        if (m_new != m[g]) {  // defer-max: wave-uniform rescale on growth
          const float corr = __expf(m[g] - m_new);
          l[g] *= corr;
#pragma unroll
          for (int e = 0; e < EPL; ++e) o[g][e] *= corr;
          m[g] = m_new;
        }
        p[g] = (s[g] == -INFINITY) ? 0.f : __expf(s[g] - m_new);
        rsum[g] = p[g];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
          rsum[g] += __shfl_xor(rsum[g], off, 64);
        l[g] += rsum[g] * (1.0f / PARTS);  // each token counted PARTS x
      }

      // ---- PV: lane accumulates its EPL output elems ------------------
#pragma unroll
      for (int t = tp; t < tp + TOKP; ++t) {
        if (t >= tile_len) break;
        float vv[EPL];
        if constexpr (sizeof(CT) == 2) {
#pragma unroll
          for (int e = 0; e < EPL; e += 2) {
            const uint32_t vr = *reinterpret_cast<const uint32_t*>(
                &v_lds[wave][t][EPL * lane + e]);
            vv[e] = bf16_to_f32((ushort)(vr & 0xffff));
            vv[e + 1] = bf16_to_f32((ushort)(vr >> 16));
          }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; e += 2) {
            const uint32_t vr = *reinterpret_cast<const ushort*>(
                &v_lds[wave][t][EPL * lane + e]);
            const floatx2 vf = __builtin_amdgcn_cvt_pk_f32_bf8(vr, false);
            vv[e] = vf.x;
            vv[e + 1] = vf.y;
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pt = __shfl(p[g], (t - tp) * PARTS, 64);
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            o[g][e] = fmaf(pt, vv[e], o[g][e]);
        }
      }
    }

    // land the prefetched tile over the one just consumed (waits only on
    // vmcnt; the reads above are earlier LDS operations of the same wave)
    if (blk_i + kWaves < blk_hi) write_tile();
  }

  // cross-wave merge through LDS
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) merge_o[wave][g][EPL * lane + e] = o[g][e];
    if (lane == 0) {
      merge_ml[wave][g][0] = m[g];
      merge_ml[wave][g][1] = l[g];
    }
  }
  __syncthreads();

  // wave w finalizes heads g = w, w+2, ... (for G<2, wave 1 idles here)
  for (int g = wave; g < G; g += kWaves) {
    float m_star = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) m_star = fmaxf(m_star, merge_ml[w][g][0]);
    float l_star = 0.f, oo[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) oo[e] = 0.f;
    if (m_star != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const float c = __expf(merge_ml[w][g][0] - m_star);
        l_star += merge_ml[w][g][1] * c;
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          oo[e] += merge_o[w][g][EPL * lane + e] * c;
      }
    }
    const int head = kh * G + g;
    if (n_splits == 1) {
      const float inv_l = 1.0f / l_star;
      ushort* oh = out + ((int64_t)b * n_q + head) * HD;
#pragma unroll
      for (int e = 0; e < EPL; e += 2) {
        uint32_t packed =
            ((uint32_t)f32_to_bf16(oo[e + 1] * inv_l) << 16) |
            f32_to_bf16(oo[e] * inv_l);
        *reinterpret_cast<uint32_t*>(&oh[EPL * lane + e]) = packed;
      }
    } else {
      // flash-decoding partials (empty splits write m=-inf, l=0, o=0)
      float* po = part_o + (((int64_t)b * n_q + head) * n_splits + split) * HD;
#pragma unroll
      for (int e = 0; e < EPL; ++e) po[EPL * lane + e] = oo[e];
      if (lane == 0) {
        float* pm = part_ml + (((int64_t)b * n_q + head) * n_splits + split) * 2;
        pm[0] = m_star;
        pm[1] = l_star;
      }
    }
  }
}

// Compile-time split bounds of the merge kernels: attention_plan.h caps
// n_splits at 16; the 8 tier keeps the common small counts at half the
// registers.
constexpr int kMergeSplitCapLo = 8;
constexpr int kMergeSplitCapHi = 16;

// Merge the flash-decoding partials of one (seq, q_head) across splits for
// N contiguous output elements of that head. `po` points at the first of
// them in split 0 (16 B aligned for N = 4, 8 B for N = 2), consecutive
// splits are HD floats apart. The result comes back bf16-rounded, packed in
// pairs. Every element's arithmetic is independent of N and of which lane
// owns it, and both merge kernels go through this one helper, so they
// produce the same bits.
//
// The partials were written by workgroups all over the chip, so every load
// here is a trip to Infinity Cache or HBM, and none of their addresses
// depends on another. All of them are issued before any arithmetic: SCAP is
// a compile-time bound on n_splits (kMergeSplitCaps), the load loop is fully
// unrolled with the split index clamped to the last real split (no branch
// between loads; the surplus copies are never used), and the arithmetic
// loop after it is guarded by s < n_splits. A runtime loop over n_splits
// instead costs one serialized round trip per load (two per split).
// Arithmetic and its order are those of the runtime loop: m* as a max over
// s, l* and o accumulated in increasing s, -inf splits skipped.
template <int N, int HD, int SCAP>
DEV_INLINE void merge_partials(const float* __restrict__ po,
                               const float* __restrict__ pml,  // [n_splits, 2]
                               const int n_splits, uint32_t (&packed)[N / 2]) {
  typedef float __attribute__((ext_vector_type(N))) vecN;
  floatx2 ml[SCAP];
  vecN pv[SCAP];
#pragma unroll
  for (int s = 0; s < SCAP; ++s) {
    const int sc = min(s, n_splits - 1);
    ml[s] = *reinterpret_cast<const floatx2*>(pml + 2 * sc);
    pv[s] = *reinterpret_cast<const vecN*>(po + sc * HD);
  }
  // keep the scheduler from holding some of the loads back behind the
  // first waits to save registers (it did, for 1 of 16 at SCAP = 8 and 12
  // of 32 at SCAP = 16)
  __builtin_amdgcn_sched_barrier(0);
  float m_star = -INFINITY;
#pragma unroll
  for (int s = 0; s < SCAP; ++s)
    if (s < n_splits) m_star = fmaxf(m_star, ml[s].x);
  float l_star = 0.f, oo[N];
#pragma unroll
  for (int e = 0; e < N; ++e) oo[e] = 0.f;
#pragma unroll
  for (int s = 0; s < SCAP; ++s) {
    // an empty (-inf) or surplus split is skipped by keeping the old sums
    // (selects, not a multiply by zero, and not a branch: a branch lets
    // the compiler sink that split's loads into it, behind a wait)
    const bool use = s < n_splits && ml[s].x != -INFINITY;
    const float c = __expf(ml[s].x - m_star);
    l_star = use ? l_star + ml[s].y * c : l_star;
#pragma unroll
    for (int e = 0; e < N; ++e) oo[e] = use ? oo[e] + pv[s][e] * c : oo[e];
  }
  const float inv_l = 1.0f / l_star;
#pragma unroll
  for (int e = 0; e < N; e += 2)
    packed[e / 2] = ((uint32_t)f32_to_bf16(oo[e + 1] * inv_l) << 16) |
                    f32_to_bf16(oo[e] * inv_l);
}

// Merge flash-decoding partials: one wave per (seq, q_head).
template <int HD, int SCAP>
__global__ void decode_merge_kernel(
    ushort* __restrict__ out,             // [B, n_q, hd]
    const float* __restrict__ part_o,     // [B, n_q, n_splits, hd]
    const float* __restrict__ part_ml,    // [B, n_q, n_splits, 2]
    const int n_q, const int n_splits, const int64_t n_bh) {
  constexpr int EPL = HD / 64;
  const int64_t bh = (int64_t)blockIdx.x * (blockDim.x / WAVE_SIZE) +
                     threadIdx.x / WAVE_SIZE;
  if (bh >= n_bh) return;
  const int lane = threadIdx.x % WAVE_SIZE;
  uint32_t packed[EPL / 2];
  merge_partials<EPL, HD, SCAP>(part_o + bh * n_splits * HD + EPL * lane,
                                part_ml + bh * n_splits * 2, n_splits, packed);
  ushort* oh = out + bh * HD;
#pragma unroll
  for (int e = 0; e < EPL; e += 2)
    *reinterpret_cast<uint32_t*>(&oh[EPL * lane + e]) = packed[e / 2];
}

// Merge + fp8 row quantization: one workgroup per sequence, covering all
// n_q heads, so the o_proj input (e4m3 bytes + row scale) comes out of the
// merge instead of a quant_fp8 launch that re-reads `out` from HBM.
// A thread owns 4 contiguous elements of the [n_q*hd] row per pass
// (HD/4 threads per head) and keeps them, bf16-rounded, in registers under
// the compile-time pass count; the row amax is taken over the bf16-ROUNDED
// values, so bytes and scale equal quant_fp8 run on `out`.
constexpr int kMergeVec = 4;
constexpr int kMergeMaxThreads = 1024;
constexpr int kMergeMaxPasses = 2;  // rows up to 1024*4*2 = 8192 elements
constexpr int kMergeRowMax = kMergeMaxThreads * kMergeVec * kMergeMaxPasses;

template <int HD, int kPasses, int SCAP>
__launch_bounds__(kMergeMaxThreads) __global__ void decode_merge_fp8_kernel(
    ushort* __restrict__ out,             // [B, n_q, hd]
    unsigned char* __restrict__ out_fp8,  // [B, n_q*hd] e4m3
    float* __restrict__ out_scale,        // [B]
    const float* __restrict__ part_o,     // [B, n_q, n_splits, hd]
    const float* __restrict__ part_ml,    // [B, n_q, n_splits, 2]
    const int n_q, const int n_splits) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int row_len = n_q * HD;
  const int nvec = row_len / kMergeVec;
  ushort* orow = out + (int64_t)b * row_len;

  uint32_t packed[kPasses][kMergeVec / 2];
  float amax = 0.f;
#pragma unroll
  for (int it = 0; it < kPasses; ++it) {
    const int i = threadIdx.x + it * blockDim.x;
    if (i < nvec) {
      const int h = (i * kMergeVec) / HD;
      const int col = (i * kMergeVec) % HD;
      const int64_t bh = (int64_t)b * n_q + h;
      merge_partials<kMergeVec, HD, SCAP>(part_o + bh * n_splits * HD + col,
                                          part_ml + bh * n_splits * 2,
                                          n_splits, packed[it]);
      *reinterpret_cast<uint2*>(orow + i * kMergeVec) =
          make_uint2(packed[it][0], packed[it][1]);
#pragma unroll
      for (int e = 0; e < kMergeVec / 2; ++e) {
        const uint32_t pk = packed[it][e];
        amax = fmaxf(amax, fabsf(bf16_to_f32((ushort)(pk & 0xffff))));
        amax = fmaxf(amax, fabsf(bf16_to_f32((ushort)(pk >> 16))));
      }
    }
  }
  const float inv_scale = row_scale_fp8(amax, red, out_scale + b);
  unsigned char* frow = out_fp8 + (int64_t)b * row_len;
#pragma unroll
  for (int it = 0; it < kPasses; ++it) {
    const int i = threadIdx.x + it * blockDim.x;
    if (i < nvec) {
      uchar4 q4;
      const uint32_t p0 = packed[it][0], p1 = packed[it][1];
      q4.x = f32_to_fp8(bf16_to_f32((ushort)(p0 & 0xffff)) * inv_scale);
      q4.y = f32_to_fp8(bf16_to_f32((ushort)(p0 >> 16)) * inv_scale);
      q4.z = f32_to_fp8(bf16_to_f32((ushort)(p1 & 0xffff)) * inv_scale);
      q4.w = f32_to_fp8(bf16_to_f32((ushort)(p1 >> 16)) * inv_scale);
      *reinterpret_cast<uchar4*>(frow + i * kMergeVec) = q4;
    }
  }
}

}  // namespace

void quant_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x);

namespace {

// The extra inputs of the raw-qkv mode (rope_cache_attention_decode)
struct RawQKV {
  torch::Tensor k, v, positions, cos_sin, slot_mapping;
};

// out_fp8 / out_scale set: also emit the e4m3 row quantization of `out`
// viewed as [B, n_q*hd] (what quant_fp8 would produce from it).
// raw non-null: q is unrotated; rotate it, rotate raw->k and write the new
// K/V rows into the caches inside the decode kernel.
//
// Instantiation set of paged_decode_kernel: the value lists of the nested
// dispatch below, G {1,2,4,5,6,8} x hd {128,256} x cache type x CAP x RAW
// (96); of the merge kernels: hd x split tier {8,16} (4), and x passes {1,2}
// for the fp8 form (8).
void decode_impl(torch::Tensor out, const c10::optional<torch::Tensor>& out_fp8,
                 const c10::optional<torch::Tensor>& out_scale, torch::Tensor q,
                 torch::Tensor k_cache, torch::Tensor v_cache,
                 torch::Tensor block_tables, torch::Tensor seq_lens,
                 double scale, int64_t window, double softcap,
                 const RawQKV* raw = nullptr) {
  const AttnShape s =
      check_paged_attention(out, q, k_cache, v_cache, block_tables, seq_lens);
  const int B = q.size(0), n_q = s.n_q, n_kv = s.n_kv, hd = s.hd;
  const int max_blocks = s.max_blocks;
  TORCH_CHECK(seq_lens.numel() >= B && block_tables.size(0) >= B);
  const bool want_fp8 = out_fp8.has_value();
  if (want_fp8) {
    TORCH_CHECK(out_scale.has_value());
    check_fp8_out(out, *out_fp8, *out_scale);
  }
  const ushort *k_new = nullptr, *v_new = nullptr;
  const int32_t* positions = nullptr;
  const float* cos_sin = nullptr;
  const int64_t* slot_mapping = nullptr;
  int64_t k_stride = 0, v_stride = 0;
  if (raw != nullptr) {
    const torch::Tensor &k = raw->k, &v = raw->v;
    TORCH_CHECK(k.dim() == 3 && v.dim() == 3);
    TORCH_CHECK(k.scalar_type() == torch::kBFloat16 &&
                v.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(k.size(0) == B && k.size(1) == n_kv && k.size(2) == hd);
    TORCH_CHECK(v.size(0) == B && v.size(1) == n_kv && v.size(2) == hd);
    TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == hd);
    TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == hd);
    TORCH_CHECK(v_cache.sizes() == k_cache.sizes() &&
                v_cache.scalar_type() == k_cache.scalar_type());
    TORCH_CHECK(k_cache.size(3) == hd);
    TORCH_CHECK(raw->positions.scalar_type() == torch::kInt32 &&
                raw->positions.is_contiguous() && raw->positions.numel() >= B);
    TORCH_CHECK(raw->slot_mapping.scalar_type() == torch::kInt64 &&
                raw->slot_mapping.is_contiguous() &&
                raw->slot_mapping.numel() >= B);
    TORCH_CHECK(raw->cos_sin.scalar_type() == torch::kFloat32 &&
                raw->cos_sin.dim() == 2 && raw->cos_sin.size(1) == hd &&
                raw->cos_sin.is_contiguous());
    // vector access: 8 B on q rows, 16 B on k / v / cos_sin / cache rows
    auto aligned = [](const torch::Tensor& t, int64_t bytes) {
      return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0 &&
             (t.dim() < 3 || t.stride(0) * t.element_size() % bytes == 0);
    };
    TORCH_CHECK(aligned(q, 8) && aligned(k, 16) && aligned(v, 16) &&
                    aligned(raw->cos_sin, 16) && aligned(k_cache, 16) &&
                    aligned(v_cache, 16),
                "rope_cache_attention_decode: misaligned q/k/v/cos_sin/cache");
    k_new = (const ushort*)k.data_ptr();
    v_new = (const ushort*)v.data_ptr();
    positions = raw->positions.data_ptr<int32_t>();
    cos_sin = raw->cos_sin.data_ptr<float>();
    slot_mapping = raw->slot_mapping.data_ptr<int64_t>();
    k_stride = k.stride(0);
    v_stride = v.stride(0);
  }
  if (B == 0) return;
  // flash-decoding split count: attn_plan::decode_n_splits (target 2048
  // workgroups, cap 16, env overrides for tuning sweeps)
  const int n_splits = attn_plan::decode_n_splits(B, n_kv, max_blocks);
  torch::Tensor part_o, part_ml;
  float *part_o_ptr = nullptr, *part_ml_ptr = nullptr;
  if (n_splits > 1) {
    auto opts =
        torch::TensorOptions().device(q.device()).dtype(torch::kFloat32);
    part_o = torch::empty({B, n_q, n_splits, (int64_t)hd}, opts);
    part_ml = torch::empty({B, n_q, n_splits, 2}, opts);
    part_o_ptr = part_o.data_ptr<float>();
    part_ml_ptr = part_ml.data_ptr<float>();
  }
  dim3 grid(B * n_kv * n_splits), block(kBlockThreads);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  // hd 256 is the gemma2 shape (G <= 2 in practice)
  dispatch_int<1, 2, 4, 5, 6, 8>(s.G, "GQA group size", [&](auto g) {
    dispatch_int<128, 256>(hd, "head dim", [&](auto hdv) {
      dispatch_bool(s.fp8_cache, [&](auto fp8) {
        dispatch_bool(softcap > 0.0, [&](auto cap) {
          dispatch_bool(raw != nullptr, [&](auto rawv) {
            using CT = std::conditional_t<decltype(fp8)::value, unsigned char,
                                          ushort>;
            hipLaunchKernelGGL(
                (paged_decode_kernel<decltype(g)::value, CT,
                                     decltype(hdv)::value, decltype(cap)::value,
                                     decltype(rawv)::value>),
                grid, block, 0, stream, (ushort*)out.data_ptr(),
                (const ushort*)q.data_ptr(), (CT*)k_cache.data_ptr(),
                (CT*)v_cache.data_ptr(), block_tables.data_ptr<int32_t>(),
                seq_lens.data_ptr<int32_t>(), (float)scale, (float)softcap,
                (int)window, n_kv, max_blocks, q.stride(0), n_splits,
                part_o_ptr, part_ml_ptr, k_new, v_new, positions, cos_sin,
                slot_mapping, k_stride, v_stride);
          });
        });
      });
    });
  });
  HIP_CHECK_KERNEL();
  if (n_splits == 1) {
    // no merge launch to fuse into: plain row quantization of `out`
    if (want_fp8) quant_fp8(*out_fp8, *out_scale, out.view({B, -1}));
    return;
  }
  static_assert(kMergeSplitCapHi == 16, "decode_n_splits caps splits at 16");
  TORCH_CHECK(n_splits <= kMergeSplitCapHi);
  // fp8 in the merge: needs a row within the fused kernel's bound
  const bool fuse_fp8 = want_fp8 && (int64_t)n_q * hd <= kMergeRowMax;
  dispatch_int<128, 256>(hd, "head dim", [&](auto hdv) {
    // split-bound tier of the merge kernels
    dispatch_bool(n_splits <= kMergeSplitCapLo, [&](auto lo) {
      constexpr int HD = decltype(hdv)::value;
      constexpr int SCAP =
          decltype(lo)::value ? kMergeSplitCapLo : kMergeSplitCapHi;
      if (fuse_fp8) {
        const int nvec = n_q * hd / kMergeVec;
        // whole waves; one pass where the row fits 1024 threads x 4 elements
        const int threads = std::min(
            kMergeMaxThreads, (nvec + WAVE_SIZE - 1) / WAVE_SIZE * WAVE_SIZE);
        dispatch_int<1, 2>(
            (nvec + threads - 1) / threads, "merge pass count", [&](auto p) {
              hipLaunchKernelGGL(
                  (decode_merge_fp8_kernel<HD, decltype(p)::value, SCAP>),
                  dim3(B), dim3(threads), 0, stream, (ushort*)out.data_ptr(),
                  (unsigned char*)out_fp8->data_ptr(),
                  out_scale->data_ptr<float>(), part_o_ptr, part_ml_ptr, n_q,
                  n_splits);
            });
      } else {
        const int64_t n_bh = (int64_t)B * n_q;
        const int wpb = 4;
        hipLaunchKernelGGL((decode_merge_kernel<HD, SCAP>),
                           dim3((uint32_t)((n_bh + wpb - 1) / wpb)),
                           dim3(wpb * WAVE_SIZE), 0, stream,
                           (ushort*)out.data_ptr(), part_o_ptr, part_ml_ptr,
                           n_q, n_splits, n_bh);
      }
    });
  });
  HIP_CHECK_KERNEL();
  // row beyond the fused kernel's bound: plain row quantization of `out`
  if (want_fp8 && !fuse_fp8) quant_fp8(*out_fp8, *out_scale, out.view({B, -1}));
}

}  // namespace

void paged_attention_decode(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor seq_lens,
                            double scale, int64_t window, double softcap) {
  decode_impl(out, c10::nullopt, c10::nullopt, q, k_cache, v_cache,
              block_tables, seq_lens, scale, window, softcap);
}

void paged_attention_decode_fp8(torch::Tensor out, torch::Tensor out_fp8,
                                torch::Tensor out_scale, torch::Tensor q,
                                torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_tables,
                                torch::Tensor seq_lens, double scale,
                                int64_t window, double softcap) {
  decode_impl(out, out_fp8, out_scale, q, k_cache, v_cache, block_tables,
              seq_lens, scale, window, softcap);
}

// rope_and_cache followed by paged_attention_decode[_fp8] for a pure-decode
// step, without the rope launch: the decode kernel rotates q and k itself
// and writes the new K/V rows. Same out / fp8 bytes / row scales / cache
// bytes as the two-op sequence. q, k and v are NOT rotated in place (the one
// difference from rope_and_cache): they are only read.
// Contract: row b with slot_mapping[b] >= 0 is a decode row, i.e. the slot
// is row (L-1) % 16 of block block_tables[b][(L-1)/16] with L = seq_lens[b].
// out_fp8 / out_scale may be None (no fp8 output).
void rope_cache_attention_decode(
    torch::Tensor out, c10::optional<torch::Tensor> out_fp8,
    c10::optional<torch::Tensor> out_scale, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor positions, torch::Tensor cos_sin,
    torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor slot_mapping,
    torch::Tensor block_tables, torch::Tensor seq_lens, double scale,
    int64_t window, double softcap) {
  const RawQKV raw{k, v, positions, cos_sin, slot_mapping};
  decode_impl(out, out_fp8, out_scale, q, k_cache, v_cache, block_tables,
              seq_lens, scale, window, softcap, &raw);
}
