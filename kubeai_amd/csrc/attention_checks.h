// Host argument checks shared by the paged-attention launchers
// (attention_decode.hip, attention_prefill.hip, attention_prefill_v2.hip).
#pragma once

#include <torch/extension.h>

#include "attention_plan.h"

// What every launcher derives from its tensors once they are validated
struct AttnShape {
  int n_q, n_kv, hd, G, max_blocks;
  bool fp8_cache;  // e5m2 cache (bf16 otherwise)
};

// q [T, n_q, hd] bf16, rows may be strided (a view into the fused qkv
// output); out [T, n_q, hd] contiguous; caches [nb, n_kv, 16, hd] contiguous,
// bf16 or e5m2; block_tables [B, max_blocks] and seq_lens [B] int32.
inline AttnShape check_paged_attention(const torch::Tensor& out,
                                       const torch::Tensor& q,
                                       const torch::Tensor& k_cache,
                                       const torch::Tensor& v_cache,
                                       const torch::Tensor& block_tables,
                                       const torch::Tensor& seq_lens) {
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
  TORCH_CHECK(out.is_contiguous());
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16);
  const bool fp8_cache = k_cache.scalar_type() == torch::kFloat8_e5m2;
  TORCH_CHECK(fp8_cache || k_cache.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(block_tables.scalar_type() == torch::kInt32);
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32);
  const int n_q = q.size(1), hd = q.size(2);
  const int n_kv = k_cache.size(1);
  const int max_blocks = block_tables.size(1);
  TORCH_CHECK(hd == 128 || hd == 256,
              "paged attention supports head_dim 128 or 256");
  TORCH_CHECK(k_cache.size(2) == attn_plan::kBlockSize,
              "paged attention supports block_size=16");
  TORCH_CHECK(n_q % n_kv == 0);
  return {n_q, n_kv, hd, n_q / n_kv, max_blocks, fp8_cache};
}

// (out_fp8, out_scale): the e4m3 row quantization of `out` viewed as
// [rows, n_q*hd], one f32 scale per row
inline void check_fp8_out(const torch::Tensor& out,
                          const torch::Tensor& out_fp8,
                          const torch::Tensor& out_scale) {
  TORCH_CHECK(out_fp8.is_contiguous() && out_scale.is_contiguous());
  TORCH_CHECK(out_fp8.scalar_type() == torch::kFloat8_e4m3fn);
  TORCH_CHECK(out_scale.scalar_type() == torch::kFloat32);
  TORCH_CHECK(out_fp8.numel() == out.numel() &&
              out_scale.numel() == out.size(0));
}
