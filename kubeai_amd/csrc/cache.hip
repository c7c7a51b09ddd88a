// Paged KV-cache write: scatter new K/V token vectors into cache blocks.
//
// Cache layout [num_blocks, n_kv, block_size, hd]: one (block, kv-head) tile
// is block_size*hd contiguous elements, the coalesced read unit for decode.
// Semantics: kubeai_amd/ops/ref.py::reshape_and_cache.
#include <torch/extension.h>

#include <type_traits>

#include "common.h"
#include "dispatch.h"

namespace {

// one 8-element vector of a row: 16 B as it is, or 8 e5m2 bytes
DEV_INLINE void store_cache_vec(ushort* p, const ushort8 v) {
  *reinterpret_cast<ushort8*>(p) = v;
}
DEV_INLINE void store_cache_vec(unsigned char* p, const ushort8 v) {
  *reinterpret_cast<uint64_t*>(p) = bf16x8_to_e5m2x8(v);
}

// CT = cache element type: ushort (bf16) or unsigned char (fp8 e5m2,
// converted while scattering)
template <typename CT>
__global__ void reshape_and_cache_kernel(
    const ushort* __restrict__ k,   // [T, n_kv, hd]
    const ushort* __restrict__ v,   // [T, n_kv, hd]
    CT* __restrict__ k_cache,       // [nb, n_kv, bs, hd]
    CT* __restrict__ v_cache,
    const int64_t* __restrict__ slot_mapping,  // [T]
    const int n_kv, const int bs, const int hd, const int64_t n_tok,
    const int64_t kv_stride) {
  // one wave per (token, kv_head); lane i copies 8 elems (hd=128 -> 2 vec/lane)
  const int64_t flat = (int64_t)blockIdx.x * (blockDim.x / WAVE_SIZE) +
                       threadIdx.x / WAVE_SIZE;
  const int64_t tok = flat / n_kv;
  if (tok >= n_tok) return;  // tail guard: slot_mapping index stays in range
  const int h = (int)(flat % n_kv);
  const int lane = threadIdx.x % WAVE_SIZE;
  const int64_t slot = slot_mapping[tok];
  if (slot < 0) return;

  const ushort8* src_k =
      reinterpret_cast<const ushort8*>(k + tok * kv_stride + (int64_t)h * hd);
  const ushort8* src_v =
      reinterpret_cast<const ushort8*>(v + tok * kv_stride + (int64_t)h * hd);
  const int64_t row = cache_row_offset(slot, bs, n_kv, h, hd);
  CT* dst_k = k_cache + row;
  CT* dst_v = v_cache + row;
  const int nvec = hd / 8;
  for (int i = lane; i < nvec; i += WAVE_SIZE) {
    const ushort8 kk = src_k[i];
    const ushort8 vv = src_v[i];
    store_cache_vec(dst_k + i * 8, kk);
    store_cache_vec(dst_v + i * 8, vv);
  }
}

}  // namespace

void reshape_and_cache(torch::Tensor k, torch::Tensor v, torch::Tensor k_cache,
                       torch::Tensor v_cache, torch::Tensor slot_mapping) {
  // k/v may be row-strided views into the fused qkv projection output
  TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == k.size(2));
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v must share row stride");
  TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == v.size(2));
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous());
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt64);
  const bool fp8_cache = k_cache.scalar_type() == torch::kFloat8_e5m2;
  TORCH_CHECK(fp8_cache || k_cache.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type());
  const int T = k.size(0), n_kv = k.size(1), hd = k.size(2);
  const int bs = k_cache.size(2);
  TORCH_CHECK(hd % 8 == 0);
  if (T == 0) return;
  const int64_t total_waves = (int64_t)T * n_kv;
  const int waves_per_block = 4;
  const int64_t blocks = (total_waves + waves_per_block - 1) / waves_per_block;
  dispatch_bool(fp8_cache, [&](auto fp8) {
    using CT = std::conditional_t<decltype(fp8)::value, unsigned char, ushort>;
    hipLaunchKernelGGL(reshape_and_cache_kernel<CT>, dim3((uint32_t)blocks),
                       dim3(waves_per_block * WAVE_SIZE), 0,
                       c10::hip::getCurrentHIPStream().stream(),
                       (const ushort*)k.data_ptr(), (const ushort*)v.data_ptr(),
                       (CT*)k_cache.data_ptr(), (CT*)v_cache.data_ptr(),
                       slot_mapping.data_ptr<int64_t>(), n_kv, bs, hd,
                       (int64_t)T, k.stride(0));
  });
  HIP_CHECK_KERNEL();
}
