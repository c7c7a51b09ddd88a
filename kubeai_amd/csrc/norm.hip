// RMSNorm kernels for gfx950.
//
// Semantics match kubeai_amd/ops/ref.py::rmsnorm / fused_add_rmsnorm
// (fp32 accumulation, bf16 IO). One workgroup (256 threads) per token row;
// bf16 loads vectorized as ushort8 (16 B/lane); the fused variant does the
// residual-add + norm in a single HBM round trip (reference analog:
// vLLM's fused_add_rms_norm — re-designed here, not ported).
//
// The row stays in registers between the two passes: the per-thread
// iteration count is a template parameter and the loops over it are fully
// unrolled with an `i < nvec` guard, so vals[] is indexed by constants only
// (a runtime-indexed array is demoted to private memory).
#include <torch/extension.h>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxIters = 8;  // supports H up to 256*8*8 = 16384

// Element mapping i = threadIdx.x + it*kBlock: each thread sums the same
// squares in the same order as a strided runtime loop would.
template <bool kFused, int kIters>
__launch_bounds__(kBlock) __global__ void rmsnorm_kernel(
    ushort* __restrict__ out,        // [T, H] bf16 (== x for fused)
    ushort* __restrict__ x,          // [T, H] bf16
    ushort* __restrict__ residual,   // [T, H] bf16 (fused only; updated)
    const ushort* __restrict__ w,    // [H] bf16
    const float eps, const int H) {
  const int row = blockIdx.x;
  ushort8* xrow = reinterpret_cast<ushort8*>(x + (int64_t)row * H);
  ushort8* rrow = kFused ? reinterpret_cast<ushort8*>(residual + (int64_t)row * H) : nullptr;
  ushort8* orow = reinterpret_cast<ushort8*>(out + (int64_t)row * H);
  const ushort8* wv = reinterpret_cast<const ushort8*>(w);
  const int nvec = H / 8;

  float vals[kIters][8];
  float ssum = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kBlock;
    if (i < nvec) {
      ushort8 xv = xrow[i];
      ushort8 rin;
      if constexpr (kFused) rin = rrow[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_to_f32(xv[j]);
        if constexpr (kFused) f += bf16_to_f32(rin[j]);
        vals[it][j] = f;
        ssum += f * f;
      }
      if constexpr (kFused) {
        // write residual' = x + residual back
        ushort8 rv;
#pragma unroll
        for (int j = 0; j < 8; ++j) rv[j] = f32_to_bf16(vals[it][j]);
        rrow[i] = rv;
      }
    }
  }
  // the norm weights do not depend on the reduction: load them above it
  ushort8 wreg[kIters];
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kBlock;
    if (i < nvec) wreg[it] = wv[i];
  }

  __shared__ float red[16];
  float total = block_reduce_sum(ssum, red);
  const float inv_rms = rsqrtf(total / (float)H + eps);

#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kBlock;
    if (i < nvec) {
      ushort8 ov;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ov[j] = f32_to_bf16(vals[it][j] * inv_rms * bf16_to_f32(wreg[it][j]));
      orow[i] = ov;
    }
  }
}

// smallest instantiated iteration count in {1, 2, 4, 8} covering the row
#define NORM_DISPATCH(nvec, LAUNCH)                   \
  do {                                                \
    const int n_it_ = ((nvec) + kBlock - 1) / kBlock; \
    if (n_it_ <= 1) { LAUNCH(1); }                    \
    else if (n_it_ <= 2) { LAUNCH(2); }               \
    else if (n_it_ <= 4) { LAUNCH(4); }               \
    else { LAUNCH(8); }                               \
  } while (0)

}  // namespace

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor weight,
             double eps) {
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  const int H = x.size(-1);
  const int T = x.numel() / H;
  TORCH_CHECK(H % 8 == 0 && H <= kBlock * 8 * kMaxIters);
#define LAUNCH_ROW(ITERS)                                                     \
  hipLaunchKernelGGL((rmsnorm_kernel<false, ITERS>), dim3(T), dim3(kBlock),   \
                     0, c10::hip::getCurrentHIPStream().stream(),             \
                     (ushort*)out.data_ptr(), (ushort*)x.data_ptr(), nullptr, \
                     (const ushort*)weight.data_ptr(), (float)eps, H)
  NORM_DISPATCH(H / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}

void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor weight, double eps) {
  TORCH_CHECK(x.is_contiguous() && residual.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  const int H = x.size(-1);
  const int T = x.numel() / H;
  TORCH_CHECK(H % 8 == 0 && H <= kBlock * 8 * kMaxIters);
#define LAUNCH_ROW(ITERS)                                                   \
  hipLaunchKernelGGL((rmsnorm_kernel<true, ITERS>), dim3(T), dim3(kBlock),  \
                     0, c10::hip::getCurrentHIPStream().stream(),           \
                     (ushort*)x.data_ptr(), (ushort*)x.data_ptr(),          \
                     (ushort*)residual.data_ptr(),                          \
                     (const ushort*)weight.data_ptr(), (float)eps, H)
  NORM_DISPATCH(H / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}
