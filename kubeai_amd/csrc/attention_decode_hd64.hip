// Paged-attention decode at head_dim 64 (Llama-3.2-1B, Qwen2 / Qwen2.5-0.5B,
// TinyLlama-class models) for gfx950.
//
// Semantics: kubeai_amd/ops/ref.py::paged_attention_decode. Scope: causal, no
// window, no softcap, bf16 or e5m2 cache, block size 16, G in {1, 2, 4, 7, 8}.
//
// The workgroup and split structure is paged_decode_kernel's
// (attention_decode.hip): grid (seq, kv head, split), 2 waves, per-wave LDS
// tile without barriers in the loop, fp32 (m, l, o) partials in the same
// layout, so decode_impl's merge kernels serve both. What differs is the
// tile. At hd 64 a 32-element lane slice is half a row, so a 16-token cache
// block fills 32 of 64 lanes in the score pass and 2 KB of a wave's loads.
// Here a wave takes TWO cache blocks (32 tokens) per step:
//  - staging: 4 vectors of K and 4 of V per lane (vectors 0, 1 from the first
//    block, 2, 3 from the second): the bytes in flight per wave of the hd-128
//    kernel. The second block of a pair that is past the split's last block is
//    not a branch around the loads: its table index is clamped to the last
//    block of the split and the loaded vectors are replaced by zeros with a
//    select.
//  - score: lane = (token lane / 2, part lane % 2); each lane dots its
//    32-element slice with v_dot2c_f32_bf16 and one shfl_xor(1) completes the
//    row: one pass over all 64 lanes scores the 32 tokens.
//  - softmax: the two blocks share one (m, l) per head, updated once per
//    tile with the defer-max rule of the hd-128 kernel.
//  - PV: half-wave h owns block h of the pair, lane % 32 owns the head_dim
//    pair (2 * (lane % 32), +1); the p of token t of that block comes from
//    lane 32 * h + 2 * t. The two halves keep separate partial sums over the
//    whole loop and are added once, in the epilogue, with shfl_xor(32).
#include <torch/extension.h>

#include <type_traits>

#include "attention_checks.h"
#include "attention_plan.h"
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int kHD = 64;
constexpr int kWaves = 2;
constexpr int kBlockThreads = kWaves * WAVE_SIZE;
constexpr int kBS = 16;            // cache block size (tokens)
constexpr int kTile = 2 * kBS;     // tokens per wave and step
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;  // v_dot2 operand
// +8 elements of row padding: rows stay 16 B (bf16) / 8 B (e5m2) aligned for
// the staging vectors and the row stride is no power of two (36 dwords at
// bf16, 18 at e5m2), so the 32 token rows of a score pass spread over banks
constexpr int kPad = 8;

// CT = cache element type: ushort (bf16) or unsigned char (e5m2, staged as
// raw bytes and converted in the dot / PV with v_cvt_pk_f32_bf8)
template <int G, typename CT>
__launch_bounds__(kBlockThreads) __global__ void paged_decode_hd64_kernel(
    ushort* __restrict__ out,            // [B, n_q, 64] bf16
    const ushort* __restrict__ q,        // [B, n_q, 64] bf16, rows q_stride
    const CT* __restrict__ k_cache,      // [nb, n_kv, 16, 64]
    const CT* __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,  // [B, max_blocks]
    const int32_t* __restrict__ seq_lens,      // [B]
    const float scale, const int n_kv, const int max_blocks,
    const int64_t q_stride, const int n_splits,
    float* __restrict__ part_o,    // [B, n_q, n_splits, 64]
    float* __restrict__ part_ml) { // [B, n_q, n_splits, 2]
  const int b = blockIdx.x / (n_kv * n_splits);
  const int rem = blockIdx.x % (n_kv * n_splits);
  const int kh = rem / n_splits;
  const int split = rem % n_splits;
  const int n_q = n_kv * G;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int L = seq_lens[b];
  const int n_blocks = (L + kBS - 1) / kBS;
  const int chunk = (n_blocks + n_splits - 1) / n_splits;
  const int blk_lo = split * chunk;
  const int blk_hi = min(n_blocks, blk_lo + chunk);

  __shared__ __attribute__((aligned(16))) CT k_lds[kWaves][kTile][kHD + kPad];
  __shared__ __attribute__((aligned(16))) CT v_lds[kWaves][kTile][kHD + kPad];
  __shared__ float merge_o[kWaves][G][kHD];
  __shared__ float merge_ml[kWaves][G][2];

  // score role: token lane / 2 of the tile, slice lane % 2 of its row
  const int tok = lane >> 1;
  const int part = lane & 1;
  // PV role: block lane / 32 of the pair, head_dim pair lane % 32
  const int half = lane >> 5;
  const int ln = lane & 31;

  // q slice of this lane's part, packed bf16 pairs
  uint32_t q_pack[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(
        q + (int64_t)b * q_stride + (int64_t)(kh * G + g) * kHD + part * 32);
#pragma unroll
    for (int i = 0; i < 16; ++i) q_pack[g][i] = qp[i];
  }

  float m[G], l[G], o[G][2];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
    o[g][0] = o[g][1] = 0.f;
  }

  // staging vector = 8 elements: 16 B (bf16) or 8 B (e5m2 bytes). A block is
  // 128 vectors, two per lane; stage_*[2 * h + j] is vector lane + 64 * j of
  // block h of the pair.
  using StageVec = std::conditional_t<sizeof(CT) == 2, ushort8, uint64_t>;
  // LDS is written as staging vectors and read back as 4- and 2-byte words:
  // may_alias keeps those reads behind the stores (see paged_decode_kernel)
  typedef StageVec __attribute__((may_alias)) LdsVec;
  StageVec stage_k[4], stage_v[4];
  const int32_t* bt = block_tables + (int64_t)b * max_blocks;

  // blk_i < blk_hi. The partner block blk_i + 1 exists inside the split or
  // not; when not, its index is clamped onto a block of the split (a valid
  // table entry) and what was loaded is dropped by a select, so the loads
  // stay unconditional.
  auto issue_loads = [&](const int blk_i) {
    const bool has1 = blk_i + 1 < blk_hi;
    const int64_t blk[2] = {bt[blk_i], bt[has1 ? blk_i + 1 : blk_hi - 1]};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t base = ((blk[h] * n_kv + kh) * kBS) * kHD;
      const StageVec* src_k = reinterpret_cast<const StageVec*>(k_cache + base);
      const StageVec* src_v = reinterpret_cast<const StageVec*>(v_cache + base);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const StageVec kk = src_k[lane + j * WAVE_SIZE];
        const StageVec vv = src_v[lane + j * WAVE_SIZE];
        const bool keep = h == 0 || has1;
        stage_k[2 * h + j] = keep ? kk : StageVec{};
        stage_v[2 * h + j] = keep ? vv : StageVec{};
      }
    }
  };
  auto write_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int vec = lane + (i & 1) * WAVE_SIZE;  // vector of the block
      const int row = (i >> 1) * kBS + vec / (kHD / 8);
      const int col = vec % (kHD / 8);
      *reinterpret_cast<LdsVec*>(&k_lds[wave][row][col * 8]) = stage_k[i];
      *reinterpret_cast<LdsVec*>(&v_lds[wave][row][col * 8]) = stage_v[i];
    }
  };

  // wave w takes the block pairs w, w + 2, ... of the split
  constexpr int kStep = 2 * kWaves;
  const int first = blk_lo + 2 * wave;
  if (first < blk_hi) {
    issue_loads(first);
    write_tile();
  }

  for (int blk_i = first; blk_i < blk_hi; blk_i += kStep) {
    const int tile_start = blk_i * kBS;
    // the tile's tokens are consecutive positions: valid ones are a prefix
    const int tile_len =
        min(blk_i + 1 < blk_hi ? kTile : kBS, L - tile_start);
    if (blk_i + kStep < blk_hi) issue_loads(blk_i + kStep);

    // ---- scores: lane computes its (token, slice) partial dot ----------
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = 0.f;
    if constexpr (sizeof(CT) == 2) {
      const uint32_t* krow =
          reinterpret_cast<const uint32_t*>(&k_lds[wave][tok][part * 32]);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bf16x2v kk = __builtin_bit_cast(bf16x2v, krow[j]);
#pragma unroll
        for (int g = 0; g < G; ++g)
          s[g] = __builtin_amdgcn_fdot2_f32_bf16(
              kk, __builtin_bit_cast(bf16x2v, q_pack[g][j]), s[g], false);
      }
    } else {
      const uint32_t* krow =
          reinterpret_cast<const uint32_t*>(&k_lds[wave][tok][part * 32]);
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
#pragma unroll
    for (int g = 0; g < G; ++g) {
      s[g] += __shfl_xor(s[g], 1, 64);  // the row's other slice
      s[g] = (tok < tile_len) ? s[g] * scale : -INFINITY;
      float tmax = s[g];
#pragma unroll
      for (int off = 2; off < 64; off <<= 1)
        tmax = fmaxf(tmax, __shfl_xor(tmax, off, 64));
      const float m_new = fmaxf(m[g], tmax);
      if (m_new != m[g]) {  // wave-uniform: rescale only when the max grows
        const float corr = __expf(m[g] - m_new);
        l[g] *= corr;
        o[g][0] *= corr;
        o[g][1] *= corr;
        m[g] = m_new;
      }
      p[g] = (s[g] == -INFINITY) ? 0.f : __expf(s[g] - m_new);
      // each token is held by its two slice lanes
      l[g] += wave_reduce_sum(p[g]) * 0.5f;
    }

    // ---- PV: half-wave h accumulates block h of the pair ---------------
    // tile_len >= 1, and block 1 never holds more valid tokens than block 0,
    // so block 0's count bounds the loop for the whole wave
    const int n_iter = min(kBS, tile_len);
#pragma unroll
    for (int t = 0; t < kBS; ++t) {
      if (t >= n_iter) break;
      const int row = half * kBS + t;
      float v0, v1;
      if constexpr (sizeof(CT) == 2) {
        const uint32_t vr =
            *reinterpret_cast<const uint32_t*>(&v_lds[wave][row][2 * ln]);
        v0 = bf16_to_f32((ushort)(vr & 0xffff));
        v1 = bf16_to_f32((ushort)(vr >> 16));
      } else {
        const uint32_t vr =
            *reinterpret_cast<const ushort*>(&v_lds[wave][row][2 * ln]);
        const floatx2 vf = __builtin_amdgcn_cvt_pk_f32_bf8(vr, false);
        v0 = vf.x;
        v1 = vf.y;
      }
      // slots of a real block past the sequence end hold whatever the cache
      // held: p is 0 there, and 0 * NaN must not reach the accumulator
      const bool ok = row < tile_len;
      v0 = ok ? v0 : 0.f;
      v1 = ok ? v1 : 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pt = __shfl(p[g], (lane & 32) + 2 * t, 64);
        o[g][0] = fmaf(pt, v0, o[g][0]);
        o[g][1] = fmaf(pt, v1, o[g][1]);
      }
    }

    // land the prefetched tile over the one just consumed (the reads above
    // are earlier LDS operations of the same wave)
    if (blk_i + kStep < blk_hi) write_tile();
  }

  // ---- epilogue: add the halves, then the waves through LDS -------------
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float o0 = o[g][0] + __shfl_xor(o[g][0], 32, 64);
    const float o1 = o[g][1] + __shfl_xor(o[g][1], 32, 64);
    if (half == 0) {
      merge_o[wave][g][2 * ln] = o0;
      merge_o[wave][g][2 * ln + 1] = o1;
    }
    if (lane == 0) {
      merge_ml[wave][g][0] = m[g];
      merge_ml[wave][g][1] = l[g];
    }
  }
  __syncthreads();

  // wave w finalizes heads g = w, w + 2, ...; lane = head_dim element
  for (int g = wave; g < G; g += kWaves) {
    float m_star = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) m_star = fmaxf(m_star, merge_ml[w][g][0]);
    float l_star = 0.f, oo = 0.f;
    if (m_star != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const float c = __expf(merge_ml[w][g][0] - m_star);
        l_star += merge_ml[w][g][1] * c;
        oo += merge_o[w][g][lane] * c;
      }
    }
    const int head = kh * G + g;
    if (n_splits == 1) {
      out[((int64_t)b * n_q + head) * kHD + lane] =
          f32_to_bf16(oo * (1.0f / l_star));
    } else {
      // flash-decoding partials (empty splits write m = -inf, l = 0, o = 0)
      const int64_t at = ((int64_t)b * n_q + head) * n_splits + split;
      part_o[at * kHD + lane] = oo;
      if (lane == 0) {
        part_ml[at * 2] = m_star;
        part_ml[at * 2 + 1] = l_star;
      }
    }
  }
}

}  // namespace

// decode_impl (attention_decode.hip) comes here at hd 64 with the shape it
// validated, the split count it planned and the partial buffers it allocated
// (null when n_splits == 1: the kernel then writes bf16 `out` itself); the
// merge launch stays there. Instantiation set of paged_decode_hd64_kernel:
// G {1,2,4,7,8} x cache type (10).
void paged_attention_decode_hd64(torch::Tensor out, torch::Tensor q,
                                 torch::Tensor k_cache, torch::Tensor v_cache,
                                 torch::Tensor block_tables,
                                 torch::Tensor seq_lens, double scale,
                                 const AttnShape& s, int n_splits,
                                 float* part_o, float* part_ml) {
  const int B = q.size(0);
  TORCH_CHECK(s.hd == kHD && attn_plan::hd64_group(s.G),
              "head_dim 64 decode: unsupported shape");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() &&
              v_cache.scalar_type() == k_cache.scalar_type() &&
              k_cache.size(3) == kHD);
  TORCH_CHECK(n_splits >= 1 && (n_splits == 1 || (part_o && part_ml)));
  // 4 B loads on q rows, 16 B (bf16) / 8 B (e5m2) vectors on cache blocks
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 4 == 0 &&
                  q.stride(0) % 2 == 0 &&
                  reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 16 == 0,
              "head_dim 64 decode: misaligned q or cache");
  dim3 grid(B * s.n_kv * n_splits), block(kBlockThreads);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 4, 7, 8>(s.G, "GQA group size", [&](auto g) {
    dispatch_bool(s.fp8_cache, [&](auto fp8) {
      using CT =
          std::conditional_t<decltype(fp8)::value, unsigned char, ushort>;
      hipLaunchKernelGGL(
          (paged_decode_hd64_kernel<decltype(g)::value, CT>), grid, block, 0,
          stream, (ushort*)out.data_ptr(), (const ushort*)q.data_ptr(),
          (const CT*)k_cache.data_ptr(), (const CT*)v_cache.data_ptr(),
          block_tables.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
          (float)scale, s.n_kv, s.max_blocks, q.stride(0), n_splits, part_o,
          part_ml);
    });
  });
  HIP_CHECK_KERNEL();
}
