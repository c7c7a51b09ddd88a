// Row kernels for gfx950: one workgroup per token row, bf16 in, fp32 math.
//   rmsnorm / fused_add_rmsnorm          -> bf16
//   rmsnorm_fp8 / fused_add_rmsnorm_fp8  -> e4m3 + row scale (qkv / gate_up)
//   silu_and_mul_fp8                     -> e4m3 + row scale (down_proj)
//   quant_fp8                            -> e4m3 + row scale (o_proj)
//   quant_fp8_div                        -> the same in division form
//                                           (Fp8Linear.forward: lm_head)
//   embed_rmsnorm_fp8                    -> rmsnorm_fp8 of gathered embedding
//                                           rows, which it also writes out
//   fused_add_rmsnorm_fp8_div            -> quant_fp8_div of the bf16 row that
//                                           fused_add_rmsnorm would write
// Semantics: kubeai_amd/ops/ref.py (rmsnorm, fused_add_rmsnorm, quant_fp8).
// The fp8 variants quantize inside the PRODUCING op, so the W8A8 path pays
// no extra launch or HBM round trip for its dynamic activation scales.
// Scale convention: common.h::row_scale_fp8 (matches torch's
// .to(float8_e4m3fn) + torch._scaled_mm rowwise scale_a).
//
// The row stays in registers between the block reductions: the per-thread
// iteration count is a template parameter and every loop over it is fully
// unrolled with an `i < nvec` guard, so vals[] is only ever indexed by
// compile-time constants (a runtime-indexed array is demoted to private
// memory, a scratch round trip on the critical path of these latency-bound
// kernels). bf16 moves as ushort8, 16 B per lane.
#include <torch/extension.h>

#include <type_traits>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int kBlock = 256;      // rows up to 16384 elems in <= 8 iterations
constexpr int kBlockWide = 512;  // rows up to 32768 elems in <= 8 iterations
constexpr int kMaxIters = 8;     // 16 iterations spill VGPRs: widen the block
constexpr int kMaxH = kBlockWide * 8 * kMaxIters;

// scale the register-held row and store it as e4m3 bytes: multiplied by
// `factor` = 448/max, or (kDiv, the division form in common.h) divided by
// `factor` = the row scale
template <int kThreads, int kIters, bool kDiv = false>
DEV_INLINE void store_row_fp8(unsigned char* __restrict__ orow,
                              const float (&vals)[kIters][8],
                              const float factor, const int nvec) {
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec)
      *reinterpret_cast<uint2*>(orow + i * 8) =
          kDiv ? quant8_fp8_div(vals[it], factor) : quant8_fp8(vals[it], factor);
  }
}

// ---- rmsnorm, optionally fused residual add, bf16 or fp8 out ----
// Element mapping i = threadIdx.x + it*kThreads: at kThreads = 256 each
// thread sums the same squares in the same order as a strided runtime loop
// would. Rows beyond 16384 elements (no model preset has one) use the
// 512-thread block, which changes the sum order.
//
// kEmbed (not fused, fp8 out): x is an embedding table [V, H] and row t reads
// table row ids[t], clamped into [0, V); the row is also written to
// `residual`, which here is a plain output (layer 0's residual stream).
// kDiv (fused, fp8 out): the fp8 epilogue is the division form, applied to
// the bf16-ROUNDED normalized row, so bytes and scales equal quant_fp8_div
// run on fused_add_rmsnorm's output. `write_rows` says whether x and
// residual are updated as fused_add_rmsnorm updates them, or left alone.
template <bool kFused, bool kFp8Out, int kThreads, int kIters,
          bool kDiv = false, bool kEmbed = false>
__launch_bounds__(kThreads) __global__ void rmsnorm_kernel(
    // [T, H] e4m3 or bf16 (== x for fused bf16)
    std::conditional_t<kFp8Out, unsigned char, ushort>* __restrict__ out,
    float* __restrict__ out_scale,  // [T] (fp8 out only)
    ushort* __restrict__ x,         // [T, H] bf16 (kEmbed: [V, H], read only)
    ushort* __restrict__ residual,  // [T, H] bf16 (fused: updated; kEmbed: out)
    const ushort* __restrict__ w,   // [H] bf16
    const float eps, const int H,
    const int32_t* __restrict__ ids = nullptr,  // [T] (kEmbed only)
    const int V = 0,                            // kEmbed only
    const bool write_rows = true) {             // kDiv only
  static_assert(!kEmbed || (kFp8Out && !kFused && !kDiv));
  static_assert(!kDiv || (kFp8Out && kFused));
  const int row = blockIdx.x;
  int64_t src = row;
  if constexpr (kEmbed) src = min(max(ids[row], 0), V - 1);
  ushort8* xrow = reinterpret_cast<ushort8*>(x + src * H);
  ushort8* rrow = (kFused || kEmbed)
                      ? reinterpret_cast<ushort8*>(residual + (int64_t)row * H)
                      : nullptr;
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
        // write residual' = x + residual back
        if (!kDiv || write_rows) {
          ushort8 rv;
#pragma unroll
          for (int j = 0; j < 8; ++j) rv[j] = f32_to_bf16(vals[it][j]);
          rrow[i] = rv;
        }
      }
      if constexpr (kEmbed) rrow[i] = xv;
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

  if constexpr (kDiv) {
    // the bf16 row of the plain fused kernel, kept in registers as the
    // values quant_fp8_div would read back
    float amax = 0.f;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = threadIdx.x + it * kThreads;
      if (i < nvec) {
        ushort8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          // (v * inv_rms) * w: association pinned for bit-compatibility
          ov[j] = f32_to_bf16(vals[it][j] * inv_rms * bf16_to_f32(wreg[it][j]));
          vals[it][j] = bf16_to_f32(ov[j]);
          amax = fmaxf(amax, fabsf(vals[it][j]));
        }
        if (write_rows) xrow[i] = ov;
      }
    }
    __syncthreads();  // red[] reuse
    const float scale = row_scale_fp8_div(amax, red, out_scale + row);
    store_row_fp8<kThreads, kIters, true>(out + (int64_t)row * H, vals, scale,
                                          nvec);
  } else if constexpr (kFp8Out) {
    // normalize in registers, track amax
    float amax = 0.f;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = threadIdx.x + it * kThreads;
      if (i < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          // v * (inv_rms * w): association pinned for bit-compatibility
          vals[it][j] *= inv_rms * bf16_to_f32(wreg[it][j]);
          amax = fmaxf(amax, fabsf(vals[it][j]));
        }
      }
    }
    __syncthreads();  // red[] reuse
    const float inv_scale = row_scale_fp8(amax, red, out_scale + row);
    store_row_fp8<kThreads, kIters>(out + (int64_t)row * H, vals, inv_scale,
                                    nvec);
  } else {
    ushort8* orow = reinterpret_cast<ushort8*>(out + (int64_t)row * H);
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = threadIdx.x + it * kThreads;
      if (i < nvec) {
        ushort8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          // (v * inv_rms) * w: association pinned for bit-compatibility
          ov[j] = f32_to_bf16(vals[it][j] * inv_rms * bf16_to_f32(wreg[it][j]));
        orow[i] = ov;
      }
    }
  }
}

// ---- max-only row ops -> fp8 ----
// A producer turns vector i of an input row into 8 floats; kInWidth is the
// input row's length in units of the output row's.
struct LoadBf16 {  // quant_fp8
  static constexpr int kInWidth = 1;
  DEV_INLINE static void load(const ushort* __restrict__ in, const int W,
                              const int i, float (&v)[8]) {
    const ushort8 xv = reinterpret_cast<const ushort8*>(in)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32(xv[j]);
  }
};

struct LoadSwiglu {  // silu(gate) * up over a packed [gate | up] row
  static constexpr int kInWidth = 2;
  DEV_INLINE static void load(const ushort* __restrict__ in, const int W,
                              const int i, float (&v)[8]) {
    const ushort8 g = reinterpret_cast<const ushort8*>(in)[i];
    const ushort8 u = reinterpret_cast<const ushort8*>(in + W)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = silu(bf16_to_f32(g[j])) * bf16_to_f32(u[j]);
  }
};

template <typename Producer, bool kDiv, int kThreads, int kIters>
__launch_bounds__(kThreads) __global__ void row_fp8_kernel(
    unsigned char* __restrict__ out,  // [T, W] fp8
    float* __restrict__ out_scale,    // [T]
    const ushort* __restrict__ xin,   // [T, kInWidth * W] bf16
    const int W) {
  const int row = blockIdx.x;
  const ushort* in = xin + (int64_t)row * Producer::kInWidth * W;
  const int nvec = W / 8;

  float vals[kIters][8];
  float amax = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = threadIdx.x + it * kThreads;
    if (i < nvec) {
      Producer::load(in, W, i, vals[it]);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(vals[it][j]));
    }
  }
  __shared__ float red[16];
  const float factor = kDiv ? row_scale_fp8_div(amax, red, out_scale + row)
                            : row_scale_fp8(amax, red, out_scale + row);
  store_row_fp8<kThreads, kIters, kDiv>(out + (int64_t)row * W, vals, factor,
                                        nvec);
}

// ---- host dispatch ----
// Picks the block width and the per-thread iteration count for a row of
// `nvec` vectors and calls launch(threads, iters) with them as
// std::integral_constants. Both policies take the smallest of 256 x {1, 2,
// 4} that covers the row (the guards make a larger count than needed
// correct, only wasteful) and differ above 1024 vectors:
//   kNorm: 256 x 8 up to 2048 vectors, then 512 x 8. The 256-thread block
//          wherever it fits keeps the sum order.
//   kMax:  512 x 4 up to 2048 vectors, then 512 x 8. A max is
//          order-independent, so the width is a free tuning choice: at the
//          llama-3-8b I = 14336 (1792 vectors) 512 x 4 traced 6.7 us
//          against 8.8 us for 256 x 8
//          (profiles/r03_decode_small_kernels.md): twice the loads in
//          flight.
enum class RowPolicy { kNorm, kMax };

template <RowPolicy kPolicy, typename Launch>
void dispatch_row(const int nvec, Launch&& launch) {
  if (nvec <= kBlock) {
    launch(Int<kBlock>{}, Int<1>{});
  } else if (nvec <= kBlock * 2) {
    launch(Int<kBlock>{}, Int<2>{});
  } else if (nvec <= kBlock * 4) {
    launch(Int<kBlock>{}, Int<4>{});
  } else if constexpr (kPolicy == RowPolicy::kNorm) {
    if (nvec <= kBlock * kMaxIters) launch(Int<kBlock>{}, Int<kMaxIters>{});
    else launch(Int<kBlockWide>{}, Int<kMaxIters>{});
  } else {
    if (nvec <= kBlockWide * 4) launch(Int<kBlockWide>{}, Int<4>{});
    else launch(Int<kBlockWide>{}, Int<kMaxIters>{});
  }
}

// x is [T, in_width * W] bf16, W the output row length
void check_row_op(const torch::Tensor& x, const int64_t W) {
  TORCH_CHECK(x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(W % 8 == 0 && W <= kMaxH);
}

// x is the [T, H] input, or (ids set) the [V, H] table its rows come from
template <bool kFused, bool kFp8Out, bool kDiv = false, bool kEmbed = false>
void launch_rmsnorm(void* out, float* out_scale, const torch::Tensor& x,
                    void* residual, const torch::Tensor& weight, double eps,
                    const torch::Tensor* ids = nullptr,
                    const bool write_rows = true) {
  const int H = x.size(-1);
  check_row_op(x, H);
  const int T = kEmbed ? ids->numel() : x.numel() / H;
  if constexpr (kDiv || kEmbed) {
    TORCH_CHECK(weight.is_contiguous() && weight.numel() == H &&
                weight.scalar_type() == torch::kBFloat16);
    if (T == 0) return;
  }
  using out_t = std::conditional_t<kFp8Out, unsigned char, ushort>;
  dispatch_row<RowPolicy::kNorm>(H / 8, [&](auto threads, auto iters) {
    constexpr int kThreads = decltype(threads)::value;
    constexpr int kIters = decltype(iters)::value;
    hipLaunchKernelGGL(
        (rmsnorm_kernel<kFused, kFp8Out, kThreads, kIters, kDiv, kEmbed>),
        dim3(T), dim3(kThreads), 0, c10::hip::getCurrentHIPStream().stream(),
        (out_t*)out, out_scale, (ushort*)x.data_ptr(), (ushort*)residual,
        (const ushort*)weight.data_ptr(), (float)eps, H,
        kEmbed ? ids->data_ptr<int32_t>() : nullptr,
        kEmbed ? (int)x.size(0) : 0, write_rows);
  });
  HIP_CHECK_KERNEL();
}

template <typename Producer, bool kDiv = false>
void launch_row_fp8(torch::Tensor& out, torch::Tensor& out_scale,
                    const torch::Tensor& x) {
  const int W = x.size(-1) / Producer::kInWidth;
  check_row_op(x, W);
  TORCH_CHECK(x.size(-1) == (int64_t)W * Producer::kInWidth);
  const int T = x.numel() / x.size(-1);
  if (T == 0) return;
  dispatch_row<RowPolicy::kMax>(W / 8, [&](auto threads, auto iters) {
    constexpr int kThreads = decltype(threads)::value;
    constexpr int kIters = decltype(iters)::value;
    hipLaunchKernelGGL((row_fp8_kernel<Producer, kDiv, kThreads, kIters>), dim3(T),
                       dim3(kThreads), 0,
                       c10::hip::getCurrentHIPStream().stream(),
                       (unsigned char*)out.data_ptr(),
                       out_scale.data_ptr<float>(),
                       (const ushort*)x.data_ptr(), W);
  });
  HIP_CHECK_KERNEL();
}

}  // namespace

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor weight,
             double eps) {
  TORCH_CHECK(out.is_contiguous());
  launch_rmsnorm<false, false>(out.data_ptr(), nullptr, x, nullptr, weight, eps);
}

void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor weight, double eps) {
  TORCH_CHECK(residual.is_contiguous());
  launch_rmsnorm<true, false>(x.data_ptr(), nullptr, x, residual.data_ptr(),
                              weight, eps);
}

void rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x,
                 torch::Tensor weight, double eps) {
  launch_rmsnorm<false, true>(out.data_ptr(), out_scale.data_ptr<float>(), x,
                              nullptr, weight, eps);
}

void fused_add_rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale,
                           torch::Tensor x, torch::Tensor residual,
                           torch::Tensor weight, double eps) {
  TORCH_CHECK(residual.is_contiguous());
  launch_rmsnorm<true, true>(out.data_ptr(), out_scale.data_ptr<float>(), x,
                             residual.data_ptr(), weight, eps);
}

// (out, out_scale) = quant_fp8_div of the row fused_add_rmsnorm would leave
// in x. write_rows: also update x and residual as fused_add_rmsnorm does;
// otherwise both are only read.
void fused_add_rmsnorm_fp8_div(torch::Tensor out, torch::Tensor out_scale,
                               torch::Tensor x, torch::Tensor residual,
                               torch::Tensor weight, double eps,
                               bool write_rows) {
  TORCH_CHECK(residual.is_contiguous() && residual.sizes() == x.sizes() &&
              residual.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(out.is_contiguous() && out.numel() == x.numel() &&
              out.element_size() == 1);
  TORCH_CHECK(out_scale.is_contiguous() &&
              out_scale.scalar_type() == torch::kFloat32 &&
              out_scale.numel() * x.size(-1) == x.numel());
  launch_rmsnorm<true, true, true>(out.data_ptr(), out_scale.data_ptr<float>(),
                                   x, residual.data_ptr(), weight, eps, nullptr,
                                   write_rows);
}

// x_out[t] = table[ids[t]] (ids clamped into the table), and (out, out_scale)
// = rmsnorm_fp8 of that row.
void embed_rmsnorm_fp8(torch::Tensor out, torch::Tensor out_scale,
                       torch::Tensor x_out, torch::Tensor ids,
                       torch::Tensor table, torch::Tensor weight, double eps) {
  TORCH_CHECK(table.dim() == 2 && table.size(0) >= 1);
  TORCH_CHECK(ids.dim() == 1 && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt32);
  const int64_t T = ids.numel(), H = table.size(1);
  TORCH_CHECK(x_out.is_contiguous() && x_out.dim() == 2 && x_out.size(0) == T &&
              x_out.size(1) == H && x_out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(out.is_contiguous() && out.numel() == T * H &&
              out.element_size() == 1);
  TORCH_CHECK(out_scale.is_contiguous() &&
              out_scale.scalar_type() == torch::kFloat32 &&
              out_scale.numel() == T);
  launch_rmsnorm<false, true, false, true>(
      out.data_ptr(), out_scale.data_ptr<float>(), table, x_out.data_ptr(),
      weight, eps, &ids);
}

void silu_and_mul_fp8(torch::Tensor out, torch::Tensor out_scale,
                      torch::Tensor x) {
  launch_row_fp8<LoadSwiglu>(out, out_scale, x);
}

void quant_fp8(torch::Tensor out, torch::Tensor out_scale, torch::Tensor x) {
  launch_row_fp8<LoadBf16>(out, out_scale, x);
}

void quant_fp8_div(torch::Tensor out, torch::Tensor out_scale,
                   torch::Tensor x) {
  launch_row_fp8<LoadBf16, true>(out, out_scale, x);
}
