// Pieces shared by the W4A8 MXFP4 kernels (mxfp4_gemm.hip, the K-split kernel
// for M <= 64, and mxfp4_gemm_tiled.hip, the output-tiled kernel above it): the
// scaled-MFMA wrapper, the constants the packed layout is built on, and the
// host check of a packed weight. The layout itself and the operand layouts of
// the instruction are described in mxfp4_gemm.hip.
#pragma once

#include <torch/extension.h>

#include <utility>

#include "common.h"
#include "dispatch.h"

namespace mxfp4 {

constexpr int kWaves = 8;    // K-split width; the scale layout is built on it
constexpr int kChunk = 128;  // k per MFMA

// The fp32 adds and multiplies of these kernels are kept out of the packed
// forms (v_pk_add_f32 and kin): the pinned result is a sequence of single IEEE
// operations, and four-wide sums and scalings are what the compiler would
// pack. The attribute names a device feature, so only the device pass sees it.
#if defined(__HIP_DEVICE_COMPILE__)
#define SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SCALAR_F32
#endif

// f(Int<0>{}), f(Int<1>{}), ...: an unrolled loop whose index is a constant
// from the start, so the register arrays it indexes never become memory
template <int... U, typename F>
DEV_INLINE void static_for(std::integer_sequence<int, U...>, F&& f) {
  (f(Int<U>{}), ...);
}
template <int N, typename F>
DEV_INLINE void static_for(F&& f) {
  static_for(std::make_integer_sequence<int, N>{}, f);
}

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// acc += A (e2m1, scaled by byte SEL of `scales`) x B (e4m3, scale 1.0)
template <int SEL>
DEV_INLINE f32x4 mfma_w4a8_sel(const i32x8 a, const i32x8 b, const f32x4 acc,
                               const int scales) {
  constexpr int kOne = 0x7f7f7f7f;  // E8M0 127 = 1.0 in every byte
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, acc, 4 /* A: e2m1 */, 0 /* B: e4m3 */, SEL, scales, 0, kOne);
}

struct Packed {
  const uint4* qp;
  const uint8_t* sp;
  int N, K, n_chunks, n_groups;
};

inline Packed check_packed(const torch::Tensor& qp, const torch::Tensor& sp,
                           const int64_t N, const int64_t K) {
  TORCH_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % 32 == 0,
              "mxfp4: need N % 16 == 0 and K % 32 == 0, got [", N, ", ", K, "]");
  TORCH_CHECK(N * K < (int64_t(1) << 40));
  TORCH_CHECK(qp.is_cuda() && sp.is_cuda() && qp.device() == sp.device(),
              "mxfp4: packed codes and scales must be on one GPU");
  TORCH_CHECK(qp.is_contiguous() && sp.is_contiguous() &&
                  qp.scalar_type() == torch::kUInt8 &&
                  sp.scalar_type() == torch::kUInt8,
              "mxfp4: packed codes and scales are contiguous uint8");
  const int64_t n_chunks = (K + kChunk - 1) / kChunk;
  const int64_t n_groups = ((n_chunks + kWaves - 1) / kWaves + 3) / 4;
  TORCH_CHECK(qp.numel() == (N / 16) * n_chunks * 64 * 16,
              "mxfp4: packed codes do not describe a [", N, ", ", K, "] weight");
  TORCH_CHECK(sp.numel() == (N / 16) * n_groups * kWaves * 64 * 4,
              "mxfp4: packed scales do not describe a [", N, ", ", K,
              "] weight");
  TORCH_CHECK((uintptr_t)qp.data_ptr() % 16 == 0 &&
                  (uintptr_t)sp.data_ptr() % 4 == 0,
              "mxfp4: packed codes must be 16-byte, scales 4-byte aligned");
  return {reinterpret_cast<const uint4*>(qp.data_ptr()),
          reinterpret_cast<const uint8_t*>(sp.data_ptr()),
          (int)N, (int)K, (int)n_chunks, (int)n_groups};
}

}  // namespace mxfp4
