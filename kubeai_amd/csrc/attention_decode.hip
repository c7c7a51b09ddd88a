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

#include "attention_plan.h"
#include "common.h"

namespace {

constexpr int kWaves = 2;  // 2 waves/workgroup: fits double-buffered tiles
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
template <int G, typename CT = ushort, int HD = 128, bool CAP = false>
__launch_bounds__(kBlockThreads) __global__ void paged_decode_kernel(
    ushort* __restrict__ out,            // [B, n_q, hd] bf16
    const ushort* __restrict__ q,        // [B, n_q, hd] bf16
    const CT* __restrict__ k_cache,      // [nb, n_kv, bs, hd]
    const CT* __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,  // [B, max_blocks]
    const int32_t* __restrict__ seq_lens,      // [B]
    const float scale, const float softcap, const int window,
    const int n_kv, const int max_blocks,
    const int64_t q_stride, const int n_splits,
    float* __restrict__ part_o,    // [B, n_q, n_splits, hd]
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

  // LDS: per-wave double-buffered KV tiles + merge scratch. Element type
  // follows the cache: bf16 stages bf16; fp8 stages the RAW e5m2 bytes
  // (half the LDS footprint/traffic) and converts during compute with the
  // native packed bf8->f32 instruction (v_cvt_pk_f32_bf8). 8-element row
  // pad keeps 8 B staging alignment and breaks bank aliasing for both
  // element widths (bf16: 68-dword stride, gcd 4; fp8: 34-dword, gcd 2).
  constexpr int PARTS = HD / 32;    // lanes per token in scoring
  constexpr int TOKP = 64 / PARTS;  // tokens scored per pass
  constexpr int EPL = HD / 64;      // output elems owned per lane
  __shared__ CT k_lds[kWaves][2][kBS][HD + kPad];
  __shared__ CT v_lds[kWaves][2][kBS][HD + kPad];
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
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(
        q + (int64_t)b * q_stride + (int64_t)(kh * G + g) * HD + part * 32);
#pragma unroll
    for (int i = 0; i < 16; ++i) q_pack[g][i] = qp[i];
  }

  float m[G], l[G], o[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }

  const int32_t* bt = block_tables + (int64_t)b * max_blocks;

  // T14 async-stage: global loads for block n+1 issue before block n's
  // compute (their latency hides under it); the register payload lands in
  // the other LDS buffer just before it is needed. Per-wave buffers ->
  // no barriers anywhere in the loop.
  // staging vector = 8 elements: 16 B (bf16) or 8 B (raw fp8 bytes)
  using StageVec = std::conditional_t<sizeof(CT) == 2, ushort8, uint64_t>;
  constexpr int NS = (kBS * HD / 8) / WAVE_SIZE;
  StageVec stage_k[NS], stage_v[NS];  // this lane's vectors of each tile

  auto issue_loads = [&](int blk_i) {
    const int64_t blk = bt[blk_i];
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
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int vec = lane + i * WAVE_SIZE;  // 8-element vector index
      const int row = vec / (HD / 8);
      const int col = vec % (HD / 8);
      *reinterpret_cast<StageVec*>(&k_lds[wave][buf][row][col * 8]) =
          stage_k[i];
      *reinterpret_cast<StageVec*>(&v_lds[wave][buf][row][col * 8]) =
          stage_v[i];
    }
  };

  const int first = blk_lo + wave;
  int cur = 0;
  if (first < blk_hi) {
    issue_loads(first);
    write_tile(0);
  }

  for (int blk_i = first; blk_i < blk_hi; blk_i += kWaves) {
    const int tile_start = blk_i * kBS;
    const int tile_len = min(kBS, L - tile_start);
    if (blk_i + kWaves < blk_hi) issue_loads(blk_i + kWaves);

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
            &k_lds[wave][cur][tok][part * 32]);
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
            &k_lds[wave][cur][tok][part * 32]);
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
                &v_lds[wave][cur][t][EPL * lane + e]);
            vv[e] = bf16_to_f32((ushort)(vr & 0xffff));
            vv[e + 1] = bf16_to_f32((ushort)(vr >> 16));
          }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; e += 2) {
            const uint32_t vr = *reinterpret_cast<const ushort*>(
                &v_lds[wave][cur][t][EPL * lane + e]);
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

    // land the prefetched tile in the other buffer (waits only on vmcnt)
    if (blk_i + kWaves < blk_hi) write_tile(cur ^ 1);
    cur ^= 1;
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

// Merge the flash-decoding partials of one (seq, q_head) across splits for
// N contiguous output elements of that head. `po` points at the first of
// them in split 0 (16 B aligned for N = 4, 8 B for N = 2), consecutive
// splits are HD floats apart. The result comes back bf16-rounded, packed in
// pairs. Every element's arithmetic is independent of N and of which lane
// owns it, and both merge kernels go through this one helper, so they
// produce the same bits.
template <int N, int HD>
DEV_INLINE void merge_partials(const float* __restrict__ po,
                               const float* __restrict__ pml,  // [n_splits, 2]
                               const int n_splits, uint32_t (&packed)[N / 2]) {
  typedef float __attribute__((ext_vector_type(N))) vecN;
  float m_star = -INFINITY;
  for (int s = 0; s < n_splits; ++s) m_star = fmaxf(m_star, pml[2 * s]);
  float l_star = 0.f, oo[N];
#pragma unroll
  for (int e = 0; e < N; ++e) oo[e] = 0.f;
  for (int s = 0; s < n_splits; ++s) {
    const float ms = pml[2 * s];
    if (ms == -INFINITY) continue;
    const float c = __expf(ms - m_star);
    l_star += pml[2 * s + 1] * c;
    const vecN pv = *reinterpret_cast<const vecN*>(po + s * HD);
#pragma unroll
    for (int e = 0; e < N; ++e) oo[e] += pv[e] * c;
  }
  const float inv_l = 1.0f / l_star;
#pragma unroll
  for (int e = 0; e < N; e += 2)
    packed[e / 2] = ((uint32_t)f32_to_bf16(oo[e + 1] * inv_l) << 16) |
                    f32_to_bf16(oo[e] * inv_l);
}

// Merge flash-decoding partials: one wave per (seq, q_head).
template <int HD = 128>
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
  merge_partials<EPL, HD>(part_o + bh * n_splits * HD + EPL * lane,
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

template <int HD, int kPasses>
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
      merge_partials<kMergeVec, HD>(part_o + bh * n_splits * HD + col,
                                    part_ml + bh * n_splits * 2, n_splits,
                                    packed[it]);
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

// out_fp8 / out_scale non-null: also emit the e4m3 row quantization of
// `out` viewed as [B, n_q*hd] (what quant_fp8 would produce from it).
void decode_impl(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                 torch::Tensor v_cache, torch::Tensor block_tables,
                 torch::Tensor seq_lens, double scale, int64_t window,
                 double softcap, torch::Tensor* out_fp8,
                 torch::Tensor* out_scale) {
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
  TORCH_CHECK(out.is_contiguous());
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(k_cache.scalar_type() == torch::kBFloat16 ||
              k_cache.scalar_type() == torch::kFloat8_e5m2);
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32);
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32);
  const int B = q.size(0), n_q = q.size(1), hd = q.size(2);
  const int n_kv = k_cache.size(1);
  const int max_blocks = block_tables.size(1);
  TORCH_CHECK(hd == 128 || hd == 256,
              "decode kernel supports head_dim 128 or 256");
  TORCH_CHECK(k_cache.size(2) == kBS, "decode kernel supports block_size=16");
  const int G = n_q / n_kv;
  TORCH_CHECK(n_q % n_kv == 0);
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
  const bool fp8_cache = k_cache.scalar_type() == torch::kFloat8_e5m2;
#define LAUNCH_CT_HD(GG, CT, HDV)                                         \
  do {                                                                    \
    if (softcap > 0.0)                                                    \
      LAUNCH_IMPL(GG, CT, HDV, true);                                     \
    else                                                                  \
      LAUNCH_IMPL(GG, CT, HDV, false);                                    \
  } while (0)
#define LAUNCH_IMPL(GG, CT, HDV, CAPV)                                    \
  hipLaunchKernelGGL((paged_decode_kernel<GG, CT, HDV, CAPV>), grid,      \
                     block, 0,                                            \
                     stream, (ushort*)out.data_ptr(),                     \
                     (const ushort*)q.data_ptr(),                         \
                     (const CT*)k_cache.data_ptr(),                       \
                     (const CT*)v_cache.data_ptr(),                       \
                     block_tables.data_ptr<int32_t>(),                    \
                     seq_lens.data_ptr<int32_t>(), (float)scale,          \
                     (float)softcap, (int)window, n_kv,                   \
                     max_blocks, q.stride(0), n_splits, part_o_ptr,       \
                     part_ml_ptr)
#define LAUNCH(GG)                                                        \
  do {                                                                    \
    if (hd == 256) {                                                      \
      /* gemma2 shapes: G <= 2 in practice, fp8 cache supported */        \
      if (fp8_cache) LAUNCH_CT_HD(GG, unsigned char, 256);                \
      else LAUNCH_CT_HD(GG, ushort, 256);                                 \
    } else if (fp8_cache) {                                               \
      LAUNCH_CT_HD(GG, unsigned char, 128);                               \
    } else {                                                              \
      LAUNCH_CT_HD(GG, ushort, 128);                                      \
    }                                                                     \
  } while (0)
  switch (G) {
    case 1: LAUNCH(1); break;
    case 2: LAUNCH(2); break;
    case 4: LAUNCH(4); break;
    case 5: LAUNCH(5); break;
    case 6: LAUNCH(6); break;
    case 8: LAUNCH(8); break;
    default: TORCH_CHECK(false, "unsupported GQA group size ", G);
  }
#undef LAUNCH
#undef LAUNCH_CT_HD
#undef LAUNCH_IMPL
  HIP_CHECK_KERNEL();
  const bool want_fp8 = out_fp8 != nullptr;
  // fp8 in the merge: needs a merge launch and a row within its bound
  const bool fuse_fp8 =
      want_fp8 && n_splits > 1 && (int64_t)n_q * hd <= kMergeRowMax;
  if (fuse_fp8) {
    const int nvec = n_q * hd / kMergeVec;
    // whole waves; one pass where the row fits 1024 threads x 4 elements
    const int threads = std::min(
        kMergeMaxThreads, (nvec + WAVE_SIZE - 1) / WAVE_SIZE * WAVE_SIZE);
    const int passes = (nvec + threads - 1) / threads;
    auto* merge = hd == 256
                      ? (passes == 1 ? decode_merge_fp8_kernel<256, 1>
                                     : decode_merge_fp8_kernel<256, 2>)
                      : (passes == 1 ? decode_merge_fp8_kernel<128, 1>
                                     : decode_merge_fp8_kernel<128, 2>);
    hipLaunchKernelGGL(merge, dim3(B), dim3(threads), 0, stream,
                       (ushort*)out.data_ptr(),
                       (unsigned char*)out_fp8->data_ptr(),
                       out_scale->data_ptr<float>(), part_o_ptr, part_ml_ptr,
                       n_q, n_splits);
    HIP_CHECK_KERNEL();
    return;
  }
  if (n_splits > 1) {
    const int64_t n_bh = (int64_t)B * n_q;
    const int wpb = 4;
    if (hd == 256)
      hipLaunchKernelGGL((decode_merge_kernel<256>),
                         dim3((uint32_t)((n_bh + wpb - 1) / wpb)),
                         dim3(wpb * WAVE_SIZE), 0, stream,
                         (ushort*)out.data_ptr(), part_o_ptr, part_ml_ptr,
                         n_q, n_splits, n_bh);
    else
      hipLaunchKernelGGL((decode_merge_kernel<128>),
                         dim3((uint32_t)((n_bh + wpb - 1) / wpb)),
                         dim3(wpb * WAVE_SIZE), 0, stream,
                         (ushort*)out.data_ptr(), part_o_ptr, part_ml_ptr,
                         n_q, n_splits, n_bh);
    HIP_CHECK_KERNEL();
  }
  // no merge launch to fuse into (n_splits == 1) or row beyond the fused
  // kernel's bound: plain row quantization of `out`
  if (want_fp8) quant_fp8(*out_fp8, *out_scale, out.view({B, -1}));
}

}  // namespace

void paged_attention_decode(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_tables, torch::Tensor seq_lens,
                            double scale, int64_t window, double softcap) {
  decode_impl(out, q, k_cache, v_cache, block_tables, seq_lens, scale, window,
              softcap, nullptr, nullptr);
}

void paged_attention_decode_fp8(torch::Tensor out, torch::Tensor out_fp8,
                                torch::Tensor out_scale, torch::Tensor q,
                                torch::Tensor k_cache, torch::Tensor v_cache,
                                torch::Tensor block_tables,
                                torch::Tensor seq_lens, double scale,
                                int64_t window, double softcap) {
  TORCH_CHECK(out_fp8.is_contiguous() && out_scale.is_contiguous());
  TORCH_CHECK(out_fp8.scalar_type() == torch::kFloat8_e4m3fn);
  TORCH_CHECK(out_scale.scalar_type() == torch::kFloat32);
  TORCH_CHECK(out_fp8.numel() == out.numel() &&
              out_scale.numel() == out.size(0));
  decode_impl(out, q, k_cache, v_cache, block_tables, seq_lens, scale, window,
              softcap, &out_fp8, &out_scale);
}
