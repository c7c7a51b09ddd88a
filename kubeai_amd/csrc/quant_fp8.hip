// Fused fp8 (OCP e4m3) quantization kernels.
//
// The W8A8 path's cost on MI355X is NOT the GEMM — it is the per-linear
// dynamic activation quantization (amax + scale + cast = extra kernel
// launches and HBM round trips). These kernels emit fp8 + per-token scales
// directly from the PRODUCING op, so the quantization is free:
//   rmsnorm_fp8 / fused_add_rmsnorm_fp8  -> feeds qkv_proj / gate_up_proj
//   silu_and_mul_fp8                     -> feeds down_proj
//   quant_fp8 (one pass)                 -> feeds o_proj (attention out)
// Scale convention: per row, scale = max(|x|)/448; y = x/scale, RNE cast
// (matches torch .to(float8_e4m3fn) + torch._scaled_mm rowwise scale_a).
#include <hip/hip_fp8.h>
#include <torch/extension.h>

#include "common.h"

namespace {

// Row kernels keep their whole row in registers between the block
// reductions. The per-thread iteration count is a template parameter and
// every loop over it is fully unrolled with an `i < nvec` guard, so vals[]
// is only ever indexed by compile-time constants: a runtime-indexed array
// is demoted to private (scratch) memory, which put a scratch round trip
// on the critical path of these latency-bound kernels.
constexpr int kBlock = 256;      // rows up to 16384 elems in <= 8 iterations
constexpr int kBlockWide = 512;  // rows up to 32768 elems in <= 8 iterations
constexpr int kMaxIters = 8;     // 16 iterations spill VGPRs: widen the block
constexpr int kMaxH = kBlockWide * 8 * kMaxIters;
// f32_to_fp8, quant8_fp8 and block_amax live in common.h (shared with the
// fp8-emitting flash-decoding merge in attention_decode.hip).

// scale the register-held row by inv_scale and store it as e4m3 bytes
template <int kThreads, int kIters>
DEV_INLINE void store_row_fp8(unsigned char* __restrict__ orow,
                              const float (&vals)[kIters][8],
                              const float inv_scale, const int nvec) {
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec)
      *reinterpret_cast<uint2*>(orow + i * 8) = quant8_fp8(vals[it], inv_scale);
  }
}

// ---- rmsnorm -> fp8 (optionally fused residual add) ----
// Element mapping i = threadIdx.x + it*kThreads: at kThreads = 256 each
// thread sums the same squares in the same order as the pre-template loop,
// so results are bit-identical for H <= 16384. Wider rows (no model preset
// has one) use the 512-thread block, which changes the sum order.
template <bool kFused, int kThreads, int kIters>
__launch_bounds__(kThreads) __global__ void rmsnorm_fp8_kernel(
    unsigned char* __restrict__ out,  // [T, H] fp8
    float* __restrict__ out_scale,    // [T]
    ushort* __restrict__ x,           // [T, H] bf16
    ushort* __restrict__ residual,    // [T, H] bf16 (fused; updated)
    const ushort* __restrict__ w,     // [H]
    const float eps, const int H) {
  const int row = blockIdx.x;
  ushort8* xrow = reinterpret_cast<ushort8*>(x + (int64_t)row * H);
  ushort8* rrow =
      kFused ? reinterpret_cast<ushort8*>(residual + (int64_t)row * H) : nullptr;
  const ushort8* wv = reinterpret_cast<const ushort8*>(w);
  const int nvec = H / 8;

  float vals[kIters][8];
  float ssum = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
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
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec) wreg[it] = wv[i];
  }

  __shared__ float red[16];
  const float total = block_reduce_sum(ssum, red);
  const float inv_rms = rsqrtf(total / (float)H + eps);

  // normalize in registers, track amax
  float amax = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        vals[it][j] *= inv_rms * bf16_to_f32(wreg[it][j]);
        amax = fmaxf(amax, fabsf(vals[it][j]));
      }
    }
  }
  __syncthreads();  // red[] reuse
  const float gmax = fmaxf(block_amax(amax, red), 1e-6f);
  const float scale = gmax / 448.0f;
  if (threadIdx.x == 0) out_scale[row] = scale;
  const float inv_scale = 448.0f / gmax;
  store_row_fp8<kThreads, kIters>(out + (int64_t)row * H, vals, inv_scale, nvec);
}

// ---- silu(gate) * up -> fp8 ----
template <int kThreads, int kIters>
__launch_bounds__(kThreads) __global__ void silu_and_mul_fp8_kernel(
    unsigned char* __restrict__ out,  // [T, I]
    float* __restrict__ out_scale,    // [T]
    const ushort* __restrict__ xin,   // [T, 2I]
    const int I) {
  const int row = blockIdx.x;
  const ushort8* gate = reinterpret_cast<const ushort8*>(xin + (int64_t)row * 2 * I);
  const ushort8* up =
      reinterpret_cast<const ushort8*>(xin + (int64_t)row * 2 * I + I);
  const int nvec = I / 8;

  float vals[kIters][8];
  float amax = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec) {
      ushort8 g = gate[i], u = up[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gf = bf16_to_f32(g[j]);
        const float s = gf / (1.0f + __expf(-gf));
        const float v = s * bf16_to_f32(u[j]);
        vals[it][j] = v;
        amax = fmaxf(amax, fabsf(v));
      }
    }
  }
  __shared__ float red[16];
  const float gmax = fmaxf(block_amax(amax, red), 1e-6f);
  const float scale = gmax / 448.0f;
  if (threadIdx.x == 0) out_scale[row] = scale;
  const float inv_scale = 448.0f / gmax;
  store_row_fp8<kThreads, kIters>(out + (int64_t)row * I, vals, inv_scale, nvec);
}

// ---- plain bf16 -> fp8 row quant (attention output) ----
template <int kThreads, int kIters>
__launch_bounds__(kThreads) __global__ void quant_fp8_kernel(
    unsigned char* __restrict__ out, float* __restrict__ out_scale,
    const ushort* __restrict__ xin, const int H) {
  const int row = blockIdx.x;
  const ushort8* xrow = reinterpret_cast<const ushort8*>(xin + (int64_t)row * H);
  const int nvec = H / 8;
  float vals[kIters][8];
  float amax = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec) {
      ushort8 xv = xrow[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf16_to_f32(xv[j]);
        vals[it][j] = f;
        amax = fmaxf(amax, fabsf(f));
      }
    }
  }
  __shared__ float red[16];
  const float gmax = fmaxf(block_amax(amax, red), 1e-6f);
  const float scale = gmax / 448.0f;
  if (threadIdx.x == 0) out_scale[row] = scale;
  const float inv_scale = 448.0f / gmax;
  store_row_fp8<kThreads, kIters>(out + (int64_t)row * H, vals, inv_scale, nvec);
}

void check_row_op(const torch::Tensor& x, int max_h) {
  TORCH_CHECK(x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.size(-1) % 8 == 0 && x.size(-1) <= max_h);
}

// Host dispatch on the per-thread iteration count: the smallest of
// {1, 2, 4, 8} that covers the row at the chosen block width (the guards
// make a larger count than needed correct, only wasteful).
#define ROW_DISPATCH_ITERS(THREADS, nvec, LAUNCH)              \
  do {                                                         \
    const int n_it_ = ((nvec) + (THREADS)-1) / (THREADS);      \
    if (n_it_ <= 1) { LAUNCH(THREADS, 1); }                    \
    else if (n_it_ <= 2) { LAUNCH(THREADS, 2); }               \
    else if (n_it_ <= 4) { LAUNCH(THREADS, 4); }               \
    else { LAUNCH(THREADS, 8); }                               \
  } while (0)

// rmsnorm: the 256-thread block wherever it fits in kMaxIters iterations
// (keeps the sum order), the wide block beyond
#define ROW_DISPATCH_NORM(nvec, LAUNCH)                        \
  do {                                                         \
    if ((nvec) <= kBlock * kMaxIters)                          \
      ROW_DISPATCH_ITERS(kBlock, nvec, LAUNCH);                \
    else                                                       \
      LAUNCH(kBlockWide, 8);                                   \
  } while (0)

// silu_and_mul_fp8 / quant_fp8 reduce with max only (order-independent), so
// their block width is a free tuning choice: the wide block above 1024
// vectors per row. At the llama-3-8b I = 14336 (1792 vectors) 512 threads
// x 4 iterations traced 6.7 us against 8.8 us for 256 x 8
// (profiles/r03_decode_small_kernels.md): twice the loads in flight.
#define ROW_DISPATCH_MAX(nvec, LAUNCH)                         \
  do {                                                         \
    if ((nvec) <= kBlock) { LAUNCH(kBlock, 1); }               \
    else if ((nvec) <= kBlock * 2) { LAUNCH(kBlock, 2); }      \
    else if ((nvec) <= kBlock * 4) { LAUNCH(kBlock, 4); }      \
    else if ((nvec) <= kBlockWide * 4) { LAUNCH(kBlockWide, 4); } \
    else { LAUNCH(kBlockWide, 8); }                            \
  } while (0)

}  // namespace

void rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x,
                 torch::Tensor weight, double eps) {
  check_row_op(x, kMaxH);
  const int H = x.size(-1);
  const int T = x.numel() / H;
#define LAUNCH_ROW(THREADS, ITERS)                                          \
  hipLaunchKernelGGL((rmsnorm_fp8_kernel<false, THREADS, ITERS>), dim3(T),  \
                     dim3(THREADS), 0,                                      \
                     c10::hip::getCurrentHIPStream().stream(),              \
                     (unsigned char*)out.data_ptr(),                        \
                     out_scale.data_ptr<float>(), (ushort*)x.data_ptr(),    \
                     nullptr, (const ushort*)weight.data_ptr(), (float)eps, \
                     H)
  ROW_DISPATCH_NORM(H / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}

void fused_add_rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale,
                           torch::Tensor x, torch::Tensor residual,
                           torch::Tensor weight, double eps) {
  check_row_op(x, kMaxH);
  TORCH_CHECK(residual.is_contiguous());
  const int H = x.size(-1);
  const int T = x.numel() / H;
#define LAUNCH_ROW(THREADS, ITERS)                                          \
  hipLaunchKernelGGL((rmsnorm_fp8_kernel<true, THREADS, ITERS>), dim3(T),   \
                     dim3(THREADS), 0,                                      \
                     c10::hip::getCurrentHIPStream().stream(),              \
                     (unsigned char*)out.data_ptr(),                        \
                     out_scale.data_ptr<float>(), (ushort*)x.data_ptr(),    \
                     (ushort*)residual.data_ptr(),                          \
                     (const ushort*)weight.data_ptr(), (float)eps, H)
  ROW_DISPATCH_NORM(H / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}

void silu_and_mul_fp8(torch::Tensor out, torch::Tensor out_scale,
                      torch::Tensor x) {
  check_row_op(x, 2 * kMaxH);
  const int I = x.size(1) / 2;
  TORCH_CHECK(I % 8 == 0 && I <= kMaxH);
  const int T = x.size(0);
  if (T == 0) return;
#define LAUNCH_ROW(THREADS, ITERS)                                          \
  hipLaunchKernelGGL((silu_and_mul_fp8_kernel<THREADS, ITERS>), dim3(T),    \
                     dim3(THREADS), 0,                                      \
                     c10::hip::getCurrentHIPStream().stream(),              \
                     (unsigned char*)out.data_ptr(),                        \
                     out_scale.data_ptr<float>(),                           \
                     (const ushort*)x.data_ptr(), I)
  ROW_DISPATCH_MAX(I / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}

void quant_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x) {
  check_row_op(x, kMaxH);
  const int H = x.size(-1);
  const int T = x.numel() / H;
  if (T == 0) return;
#define LAUNCH_ROW(THREADS, ITERS)                                          \
  hipLaunchKernelGGL((quant_fp8_kernel<THREADS, ITERS>), dim3(T),           \
                     dim3(THREADS), 0,                                      \
                     c10::hip::getCurrentHIPStream().stream(),              \
                     (unsigned char*)out.data_ptr(),                        \
                     out_scale.data_ptr<float>(),                           \
                     (const ushort*)x.data_ptr(), H)
  ROW_DISPATCH_MAX(H / 8, LAUNCH_ROW);
#undef LAUNCH_ROW
  HIP_CHECK_KERNEL();
}
