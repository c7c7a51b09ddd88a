// Fused NeoX rotary embedding + paged KV-cache write, one launch.
//
// Equals rope (rope.hip) followed by reshape_and_cache (cache.hip), bit for
// bit: q and k are rotated in place, the rotated (bf16-rounded) k and the
// untouched v of every token with slot >= 0 are scattered into the cache.
// The unfused pair re-read k and v from HBM in a second launch just to copy
// them; here the wave that rotates a k head also writes its cache row.
//
// Grid: one wave per (token, head) over n_q + 2*n_kv heads:
//   head <  n_q           q head: rotate in place
//   head <  n_q + n_kv    k head: rotate in place, cache row if slot >= 0
//   otherwise             v head: copy to the cache row if slot >= 0
// Tokens with slot -1 (graph pad rows, dropped tokens) are still rotated
// and write nothing to the cache. q, k and v carry independent row strides
// (views into the fused qkv buffer, or separately contiguous tensors).
#include <torch/extension.h>

#include <type_traits>

#include "common.h"
#include "dispatch.h"

namespace {

DEV_INLINE void store_cache_elem(ushort* p, ushort bf) { *p = bf; }
DEV_INLINE void store_cache_elem(unsigned char* p, ushort bf) {
  *p = f32_to_e5m2(bf16_to_f32(bf));
}

// CT = cache element type: ushort (bf16) or unsigned char (fp8 e5m2)
template <typename CT>
__global__ void rope_and_cache_kernel(
    ushort* __restrict__ q,        // [T, n_q, hd]
    ushort* __restrict__ k,        // [T, n_kv, hd]
    const ushort* __restrict__ v,  // [T, n_kv, hd]
    CT* __restrict__ k_cache,      // [nb, n_kv, bs, hd]
    CT* __restrict__ v_cache,
    const int32_t* __restrict__ positions,     // [T]
    const float* __restrict__ cos_sin,         // [max_pos, hd]
    const int64_t* __restrict__ slot_mapping,  // [T]
    const int n_q, const int n_kv, const int hd, const int bs,
    const int64_t n_tok, const int64_t q_stride, const int64_t k_stride,
    const int64_t v_stride) {
  const int n_heads = n_q + 2 * n_kv;
  const int64_t flat = (int64_t)blockIdx.x * (blockDim.x / WAVE_SIZE) +
                       threadIdx.x / WAVE_SIZE;
  const int64_t tok = flat / n_heads;
  if (tok >= n_tok) return;
  const int head = (int)(flat % n_heads);
  const int lane = threadIdx.x % WAVE_SIZE;

  if (head >= n_q + n_kv) {
    // ---- v head: 8-element vector copy into the cache row ----
    const int64_t slot = slot_mapping[tok];
    if (slot < 0) return;
    const int h = head - n_q - n_kv;
    const ushort8* src =
        reinterpret_cast<const ushort8*>(v + tok * v_stride + (int64_t)h * hd);
    CT* dst = v_cache + cache_row_offset(slot, bs, n_kv, h, hd);
    const int nvec = hd / 8;
    for (int i = lane; i < nvec; i += WAVE_SIZE) {
      const ushort8 vv = src[i];
      if constexpr (sizeof(CT) == 2) {
        reinterpret_cast<ushort8*>(dst)[i] = vv;
      } else {
        // bf16x8_to_e5m2x8, spelled out: through the helper the compiler
        // schedules this kernel differently (profiles/r06_launch_dispatch.md)
        uint64_t vo = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          vo |= (uint64_t)f32_to_e5m2(bf16_to_f32((ushort)vv[j])) << (8 * j);
        reinterpret_cast<uint64_t*>(dst)[i] = vo;
      }
    }
    return;
  }

  // ---- q / k head: lane i rotates the pair (i, i + hd/2) ----
  const int half = hd / 2;
  const bool is_k = head >= n_q;
  const int pos = positions[tok];
  const float* cs = cos_sin + (int64_t)pos * hd;
  ushort* base = is_k ? k + tok * k_stride + (int64_t)(head - n_q) * hd
                      : q + tok * q_stride + (int64_t)head * hd;
  CT* dst = nullptr;
  if (is_k) {
    const int64_t slot = slot_mapping[tok];
    if (slot >= 0)
      dst = k_cache + cache_row_offset(slot, bs, n_kv, head - n_q, hd);
  }
  for (int i = lane; i < half; i += WAVE_SIZE) {
    const float c = cs[i];
    const float s = cs[half + i];
    const float x1 = bf16_to_f32(base[i]);
    const float x2 = bf16_to_f32(base[half + i]);
    ushort o1, o2;
    rope_rotate_pair(x1, x2, c, s, o1, o2);
    base[i] = o1;
    base[half + i] = o2;
    if (dst != nullptr) {
      store_cache_elem(dst + i, o1);
      store_cache_elem(dst + half + i, o2);
    }
  }
}

}  // namespace

void rope_and_cache(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor positions, torch::Tensor cos_sin,
                    torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor slot_mapping) {
  // q/k/v may be row-strided views into the fused qkv projection output
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3);
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == q.size(2));
  TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == k.size(2));
  TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == v.size(2));
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
              k.scalar_type() == torch::kBFloat16 &&
              v.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(positions.scalar_type() == torch::kInt32);
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32);
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes());
  const bool fp8_cache = k_cache.scalar_type() == torch::kFloat8_e5m2;
  TORCH_CHECK(fp8_cache || k_cache.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type());
  const int T = q.size(0);
  const int n_q = q.size(1), n_kv = k.size(1), hd = q.size(2);
  TORCH_CHECK(hd == 128 || hd == 256,
              "rope_and_cache supports head_dim 128 or 256");
  TORCH_CHECK(k.size(0) == T && v.size(0) == T && k.size(2) == hd);
  TORCH_CHECK(v.size(1) == n_kv && v.size(2) == hd);
  TORCH_CHECK(cos_sin.size(1) == hd);
  TORCH_CHECK(k_cache.size(1) == n_kv && k_cache.size(3) == hd);
  TORCH_CHECK(positions.numel() >= T && slot_mapping.numel() >= T);
  // 16 B vector access on v rows / cache rows
  TORCH_CHECK(v.stride(0) % 8 == 0 && v.storage_offset() % 8 == 0);
  const int bs = k_cache.size(2);
  if (T == 0) return;
  const int64_t total_waves = (int64_t)T * (n_q + 2 * n_kv);
  const int waves_per_block = 4;  // 256 threads
  const int64_t blocks = (total_waves + waves_per_block - 1) / waves_per_block;
  dispatch_bool(fp8_cache, [&](auto fp8) {
    using CT = std::conditional_t<decltype(fp8)::value, unsigned char, ushort>;
    hipLaunchKernelGGL(
        rope_and_cache_kernel<CT>, dim3((uint32_t)blocks),
        dim3(waves_per_block * WAVE_SIZE), 0,
        c10::hip::getCurrentHIPStream().stream(), (ushort*)q.data_ptr(),
        (ushort*)k.data_ptr(), (const ushort*)v.data_ptr(),
        (CT*)k_cache.data_ptr(), (CT*)v_cache.data_ptr(),
        positions.data_ptr<int32_t>(), cos_sin.data_ptr<float>(),
        slot_mapping.data_ptr<int64_t>(), n_q, n_kv, hd, bs, (int64_t)T,
        q.stride(0), k.stride(0), v.stride(0));
  });
  HIP_CHECK_KERNEL();
}
