// Common helpers for kubeai_amd gfx950 (CDNA4) kernels.
//
// Conventions (see /opt/skills/guides/cdna_hip_programming.md):
//  - wave = 64 lanes, hard-coded.
//  - bf16 global loads are vectorized as ushort4/ushort8 (hipcc does not
//    auto-vectorize scalar bf16 loads).
//  - fp32 accumulation everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_fp8.h>
#include <stdint.h>
#include <c10/hip/HIPStream.h>

#define WAVE_SIZE 64
#define DEV_INLINE __device__ __forceinline__

typedef __hip_bfloat16 bf16_t;

// 16-byte vector of 8 bf16 values (one coalesced lane-load).
typedef ushort __attribute__((ext_vector_type(8))) ushort8;
typedef ushort __attribute__((ext_vector_type(4))) ushort4_t;
typedef float __attribute__((ext_vector_type(4))) float4_t;

DEV_INLINE float bf16_to_f32(ushort u) {
  union {
    uint32_t i;
    float f;
  } c;
  c.i = ((uint32_t)u) << 16;
  return c.f;
}

DEV_INLINE ushort f32_to_bf16(float f) {
  // round-to-nearest-even, matching PyTorch's bf16 cast
  union {
    float f;
    uint32_t i;
  } c;
  c.f = f;
  uint32_t x = c.i;
  uint32_t rb = ((x >> 16) & 1u) + 0x7fffu;
  x += rb;
  return (ushort)(x >> 16);
}

// ---------------- fp8 e5m2 KV-cache element (OCP bf8) ----------------
// e5m2 [s eeeee mm] -> f32 by bit widening: bias 15 -> 127. Matches
// torch.float8_e5m2 exactly incl. subnormals/inf/nan (pure exponent
// remap; subnormals handled by normalizing the 2-bit mantissa).

DEV_INLINE float e5m2_to_f32(unsigned char b) {
  const uint32_t s = ((uint32_t)b & 0x80u) << 24;
  uint32_t e = (b >> 2) & 0x1fu;
  uint32_t m = b & 0x3u;
  uint32_t out;
  if (e == 0) {
    if (m == 0) {
      out = s;  // +-0
    } else {
      // subnormal: value = m * 2^-16; normalize
      int shift = (m & 2u) ? 0 : 1;  // m=2,3 -> msb at bit1; m=1 -> bit0
      e = 127 - 15 + 1 - 1 - shift;  // 2^-15 / 2^-16
      m = (m << (shift + 1)) & 0x3u;  // drop the implicit leading 1
      out = s | (e << 23) | (m << 21);
    }
  } else if (e == 0x1fu) {
    out = s | 0x7f800000u | (m << 21);  // inf / nan
  } else {
    out = s | ((e - 15u + 127u) << 23) | (m << 21);
  }
  union { uint32_t i; float f; } c;
  c.i = out;
  return c.f;
}

// native 2 x f32 vector, the result type of the packed bf8->f32 convert
// (v_cvt_pk_f32_bf8: one instruction turns 2 e5m2 bytes into 2 floats)
typedef float floatx2 __attribute__((ext_vector_type(2)));

// 8 packed e5m2 bytes -> 8 bf16 values (one staging unit).
//
// Route: e5m2 is bit-identical to the TOP BYTE of an IEEE fp16, so
// fp16 = byte<<8 (pure integer move); fp16 -> f32 is one hardware cvt;
// f32 -> bf16 truncates losslessly (every e5m2 value, subnormals and
// inf/nan included, is exactly representable in bf16).
//
// Deliberately NOT via __builtin_amdgcn_cvt_pk_f32_bf8 + bit-level
// truncation: this toolchain mis-simplifies bit manipulation of that
// intrinsic's result (low mantissa bit folded to zero — 129/256 byte
// values corrupt, device-verified in scripts/dbg_cvt.hip; an opaque
// asm barrier does not stop it). Arithmetic (fadd/fma) consumers of
// cvt_pk_f32_bf8 are fine — the decode kernel keeps using it.
DEV_INLINE ushort8 e5m2x8_to_bf16x8(uint64_t raw) {
  ushort8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const ushort h = (ushort)((raw >> (8 * j)) << 8);
    const float f = __half2float(__builtin_bit_cast(__half, h));
    out[j] = (ushort)(__builtin_bit_cast(uint32_t, f) >> 16);
  }
  return out;
}

DEV_INLINE unsigned char f32_to_e5m2(float x) {
  // RNE with saturation to max finite (K/V magnitudes stay far below
  // e5m2's 57344 ceiling in practice)
  return (unsigned char)__hip_cvt_float_to_fp8(x, __HIP_SATFINITE, __HIP_E5M2);
}

// 8 bf16 values -> 8 packed e5m2 bytes (the inverse staging unit: what a
// cache write stores for one 16 B vector of a K/V row). rope_and_cache_kernel
// and the decode kernel's RAW store spell the same loop inline: through this
// call the compiler schedules them differently
// (profiles/r06_launch_dispatch.md).
DEV_INLINE uint64_t bf16x8_to_e5m2x8(const ushort8 v) {
  uint64_t out = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    out |= (uint64_t)f32_to_e5m2(bf16_to_f32((ushort)v[j])) << (8 * j);
  return out;
}

// ---------------- paged KV cache ----------------
// Element offset of the row of `slot` for kv head `head` in a cache laid out
// [num_blocks, n_kv, bs, hd]: block slot / bs, row slot % bs.
DEV_INLINE int64_t cache_row_offset(const int64_t slot, const int bs,
                                    const int n_kv, const int head,
                                    const int hd) {
  return (((slot / bs) * n_kv + head) * bs + slot % bs) * hd;
}

// ---------------- NeoX rotary pair ----------------
// Rotates the pair (x1, x2) = (x[i], x[i + hd/2]) by (c, s) and rounds to
// bf16. Every rotary kernel goes through this one expression, and the
// expression spells its own contraction: the x2 products are rounded, the
// x1 products are fused onto them. Left to the compiler (x1 * c - x2 * s,
// x2 * c + x1 * s under -ffp-contract=fast) which product of each sum gets
// fused depends on the surrounding code: rope_kernel and the bf16-cache
// rope_and_cache_kernel came out in exactly the form below, the fp8-cache
// rope_and_cache_kernel and the decode kernel's raw-qkv prologue fused the
// x2 * c product of o2 instead, which is one bf16 ulp apart in about one
// element in 10^5.
DEV_INLINE void rope_rotate_pair(const float x1, const float x2, const float c,
                                 const float s, ushort& o1, ushort& o2) {
#pragma clang fp contract(off)
  const float x2s = x2 * s;
  const float x2c = x2 * c;
  o1 = f32_to_bf16(__builtin_fmaf(x1, c, -x2s));
  o2 = f32_to_bf16(__builtin_fmaf(x1, s, x2c));
}

// ---------------- wave reductions (64-wide) ----------------

DEV_INLINE float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

DEV_INLINE float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Block-level sum reduce across up to 16 waves; `smem` must hold >= 16 floats.
// Every thread returns the total.
DEV_INLINE float block_reduce_sum(float v, float* smem) {
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int n_waves = (blockDim.x + WAVE_SIZE - 1) / WAVE_SIZE;
  v = wave_reduce_sum(v);
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w)
    if (w < n_waves) total += smem[w];
  return total;
}

// block-wide amax over non-negative per-thread partials, up to 16 waves
// (smem >= 16 floats). Every thread returns the maximum.
DEV_INLINE float block_amax(float v, float* smem) {
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int n_waves = (blockDim.x + WAVE_SIZE - 1) / WAVE_SIZE;
  v = wave_reduce_max(v);
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  float m = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w)
    if (w < n_waves) m = fmaxf(m, smem[w]);
  return m;
}

// ---------------- fp8 e4m3 row quantization ----------------
// Scale convention: per row, scale = max(|x|, 1e-6)/448; y = x * (448/max),
// RNE cast with saturation. Every fp8 producer goes through these helpers.
DEV_INLINE unsigned char f32_to_fp8(float x) {
  return (unsigned char)__hip_cvt_float_to_fp8(x, __HIP_SATFINITE, __HIP_E4M3);
}

// 8 floats * inv_scale -> 8 packed e4m3 bytes
DEV_INLINE uint2 quant8_fp8(const float (&f)[8], const float inv_scale) {
  uchar2 packed[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    packed[j].x = f32_to_fp8(f[2 * j] * inv_scale);
    packed[j].y = f32_to_fp8(f[2 * j + 1] * inv_scale);
  }
  return *reinterpret_cast<uint2*>(packed);
}

// Per-thread partial amax -> row scale: block amax, clamped at 1e-6;
// thread 0 writes *scale_out = max/448; every thread returns 448/max, the
// factor the row is multiplied by before the e4m3 cast. The one place the
// scale arithmetic lives (`smem` as for block_amax).
DEV_INLINE float row_scale_fp8(const float amax, float* smem,
                               float* __restrict__ scale_out) {
  const float gmax = fmaxf(block_amax(amax, smem), 1e-6f);
  if (threadIdx.x == 0) *scale_out = gmax / 448.0f;
  return 448.0f / gmax;
}

// Division form of the same quantization: the expression Fp8Linear.forward
// (engine/quant.py) evaluates with torch ops on the GPU,
//   scale = max(|x|, 1e-6) / 448;  y = clamp(x / scale, -448, 448), RNE cast.
// x / scale and x * (448/max) round differently, so a linear whose outputs
// are pinned to one form cannot move to the other. torch divides a GPU tensor
// by a host scalar as a multiplication by the scalar's fp32 reciprocal; the
// per-element x / scale is a true fp32 division.
// Thread 0 writes *scale_out; every thread returns the scale.
DEV_INLINE float row_scale_fp8_div(const float amax, float* smem,
                                   float* __restrict__ scale_out) {
  const float gmax = fmaxf(block_amax(amax, smem), 1e-6f);
  const float scale = gmax * (float)(1.0 / 448.0);
  if (threadIdx.x == 0) *scale_out = scale;
  return scale;
}

// 8 floats / scale, clamped -> 8 packed e4m3 bytes
DEV_INLINE uint2 quant8_fp8_div(const float (&f)[8], const float scale) {
  uchar2 packed[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    packed[j].x =
        f32_to_fp8(fminf(fmaxf(f[2 * j] / scale, -448.0f), 448.0f));
    packed[j].y =
        f32_to_fp8(fminf(fmaxf(f[2 * j + 1] / scale, -448.0f), 448.0f));
  }
  return *reinterpret_cast<uint2*>(packed);
}

// ---------------- activations ----------------
DEV_INLINE float silu(const float x) { return x / (1.0f + __expf(-x)); }

// ---------------- hash RNG (kernel/ref-identical spec) ----------------
//
// Sampling uses a counter-based hash RNG so the HIP kernel and the PyTorch
// reference produce bit-identical streams: u64 = splitmix64(key*M ^ idx).
DEV_INLINE uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// uniform in (0, 1]
DEV_INLINE float hash_uniform(uint64_t key, uint64_t idx) {
  uint64_t h = splitmix64(key ^ (idx * 0xd1342543de82ef95ull));
  // take top 24 bits -> (0,1] to keep -log well-defined
  uint32_t m = (uint32_t)(h >> 40);
  return ((float)m + 1.0f) * (1.0f / 16777216.0f);
}

#define HIP_CHECK_KERNEL()                                    \
  do {                                                        \
    hipError_t e = hipGetLastError();                         \
    if (e != hipSuccess) {                                    \
      TORCH_CHECK(false, "HIP kernel launch failed: ",        \
                  hipGetErrorString(e));                      \
    }                                                         \
  } while (0)
