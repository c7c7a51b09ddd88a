// Device pieces shared by the W4A16 kernels (int4_gemm.hip, int4_moe.hip): the
// in-register dequantization, the K-split chunk loop and its reduction. The
// packed layout and the MFMA slot assignment are described in int4_gemm.hip.
//
// Both GEMM kernels run int4_chunk_loop and int4_reduce_store; they differ
// only in where a lane's x rows and a tile's y rows come from. The value of
// one output row therefore does not depend on which kernel computed it, nor
// on MT, NT or the other rows: each wave sums its chunks wave, wave + 8, ...
// in order and the 8 partials are added in wave order.
#pragma once

#include <torch/extension.h>

#include "common.h"

namespace w4a16 {

constexpr int kWaves = 8;          // K-split width of the fused kernels
constexpr int kChunk = 128;        // k per (wave, iteration)

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// 8 codes of one word -> 8 bf16 weights. 0x4300 | q is the bf16 (and, shifted,
// the fp32) encoding of 128 + q; zf = 128 + z, so the subtraction is exact and
// the product is float(q - z) * float(s) itself, the sign of a zero included
// (an fma against a pre-multiplied zero point would lose it for s < 0). The
// float -> bf16 conversion is the round-to-nearest-even v_cvt_pk_bf16_f32.
DEV_INLINE bf16x8 dequant8(const uint32_t word, const float zf, const float s) {
  u32x4 out;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    f32x2 w;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * p + h;
      const uint32_t bits = 0x43000000u | (((word >> (4 * j)) & 0xFu) << 16);
      w[h] = (__builtin_bit_cast(float, bits) - zf) * s;
    }
    out[p] = __builtin_bit_cast(uint32_t, __builtin_convertvector(w, bf16x2));
  }
  return __builtin_bit_cast(bf16x8, out);
}

// scale and (128 + zero) of row nl of `tile` in group gi
DEV_INLINE void load_scale_zero(const __half* __restrict__ sp,
                                const uint8_t* __restrict__ zp,
                                const int64_t tile, const int n_groups,
                                const int gi, const int nl, float& s,
                                float& zf) {
  const int64_t row = tile * n_groups + gi;
  s = __half2float(sp[row * 16 + nl]);
  const uint32_t zb = zp[row * 8 + (nl >> 1)];
  zf = 128.0f + (float)((zb >> (4 * (nl & 1))) & 0xFu);
}

// The chunk loop of one workgroup: acc[nt][mt] += x rows of tile mt times
// column tile tile0 + nt, over this wave's chunks wave, wave + kWaves, ...
// xrow[mt] is the lane's row of x in row tile mt; nl = lane & 15 picks the
// row and the column, kq = lane >> 4 the quarter of the chunk.
// MT: 16-row tiles of x the accumulator holds. LT <= MT: the tiles that have
// rows; the others load no x and issue no MFMA. NT: 16-column tiles of W per
// workgroup; the x fragments of a chunk are loaded once and multiplied
// against all NT.
//
// This wave's i-th chunk is wave + i * kWaves. The loop is a two-stage
// software pipeline, since a wave that waits for each chunk's loads before
// it issues the next spends its time on HBM round trips: the codes, scales
// and zeros of all NT tiles are fetched kAhead chunks ahead into a register
// ring (kAhead * NT = 4 code loads in flight per lane), the x fragments one
// chunk ahead into the other half of a double buffer. All guards on
// `chunk < n_chunks` are wave-uniform. The MFMAs need the whole wave, so a
// lane in the zero padding of the last chunk (k >= K) stays in with zero A
// and B fragments: it reads k = 0 (in bounds) and multiplies by a zero
// scale.
template <int MT, int LT, int NT, int G>
DEV_INLINE void int4_chunk_loop(f32x4 (&acc)[NT][MT],
                                const ushort* (&xrow)[MT],
                                const uint4* __restrict__ qp,
                                const __half* __restrict__ sp,
                                const uint8_t* __restrict__ zp,
                                const int tile0, const int K,
                                const int n_chunks, const int wave,
                                const int lane, const int nl, const int kq) {
  constexpr int kAhead = 4 / NT;
  uint4 ring_c[kAhead][NT];
  float ring_s[kAhead][NT], ring_zf[kAhead][NT];
  bf16x8 a[2][LT][4];

  auto lane_k = [&](const int chunk, bool& live) {
    const int k_lane = chunk * kChunk + kq * 32;
    live = k_lane < K;
    return live ? k_lane : 0;
  };
  auto fetch_codes = [&](const int i, const int slot) {
    const int chunk = wave + i * kWaves;
    if (chunk >= n_chunks) return;
    bool live;
    const int k0 = lane_k(chunk, live);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int64_t tile = tile0 + nt;
      ring_c[slot][nt] = qp[(tile * n_chunks + chunk) * 64 + lane];
      load_scale_zero(sp, zp, tile, K / G, k0 / G, nl, ring_s[slot][nt],
                      ring_zf[slot][nt]);
      if (!live) ring_s[slot][nt] = 0.f;
    }
  };
  auto fetch_x = [&](const int i, const int buf) {
    const int chunk = wave + i * kWaves;
    if (chunk >= n_chunks) return;
    bool live;
    const int k0 = lane_k(chunk, live);
#pragma unroll
    for (int mt = 0; mt < LT; ++mt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[buf][mt][t] = *reinterpret_cast<const bf16x8*>(xrow[mt] + k0 + 8 * t);
        if (!live) a[buf][mt][t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
  };

#pragma unroll
  for (int u = 0; u < kAhead; ++u) fetch_codes(u, u);
  fetch_x(0, 0);
  const int n_iter = (n_chunks - wave + kWaves - 1) / kWaves;
  // unrolled by 2 * kAhead: ring slot and x buffer of each step are static
  for (int i0 = 0; i0 < n_iter; i0 += 2 * kAhead) {
#pragma unroll
    for (int u = 0; u < 2 * kAhead; ++u) {
      const int i = i0 + u;
      if (i < n_iter) {
        const int slot = u % kAhead;
        uint4 c[NT];
        float s[NT], zf[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          c[nt] = ring_c[slot][nt];
          s[nt] = ring_s[slot][nt];
          zf[nt] = ring_zf[slot][nt];
        }
        fetch_x(i + 1, (u + 1) & 1);
        fetch_codes(i + kAhead, slot);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const uint32_t words[4] = {c[nt].x, c[nt].y, c[nt].z, c[nt].w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const bf16x8 b = dequant8(words[t], zf[nt], s[nt]);
#pragma unroll
            for (int mt = 0; mt < LT; ++mt)
              acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[u & 1][mt][t], b, acc[nt][mt], 0, 0, 0);
          }
        }
      }
    }
  }
}

// K-split reduction, one column tile at a time through the same LDS: every
// wave parks its partial tile; the MT * 4 accumulator registers are then
// dealt out to the waves, and each lane sums its register's kWaves partials
// in wave order. Row r of the workgroup's tiles is stored where rows.stored(r),
// to row rows.row(r) of y.
template <int MT, int NT, typename Rows>
DEV_INLINE void int4_reduce_store(
    ushort* __restrict__ y, const f32x4 (&acc)[NT][MT],
    float (&part)[kWaves][MT][4][WAVE_SIZE], const int N, const int tile0,
    const int wave, const int lane, const int nl, const int kq,
    const Rows rows) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (nt > 0) __syncthreads();  // the previous tile's partials are consumed
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[wave][mt][i][lane] = acc[nt][mt][i];
    __syncthreads();
    // C layout: lane holds rows (lane >> 4) * 4 + i, column lane & 15
    for (int e = wave; e < MT * 4; e += kWaves) {
      const int mt = e >> 2, i = e & 3;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += part[w][mt][i][lane];
      const int row = mt * 16 + kq * 4 + i;
      if (rows.stored(row))
        y[(int64_t)rows.row(row) * N + (tile0 + nt) * 16 + nl] =
            f32_to_bf16(sum);
    }
  }
}

struct Packed {
  const uint4* qp;
  const __half* sp;
  const uint8_t* zp;
  int N, K, G, n_chunks;
};

inline void check_shape(const int64_t N, const int64_t K, const int64_t G) {
  TORCH_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % 32 == 0 && G > 0 &&
                  K % G == 0,
              "int4: need N % 16 == 0, K % 32 == 0, K % group == 0");
  TORCH_CHECK(N * K < (int64_t(1) << 40));
}

inline Packed check_packed(const torch::Tensor& qp, const torch::Tensor& sp,
                           const torch::Tensor& zp, const int64_t N,
                           const int64_t K, const int64_t G) {
  TORCH_CHECK(qp.is_cuda() && sp.is_cuda() && zp.is_cuda());
  TORCH_CHECK(qp.is_contiguous() && sp.is_contiguous() && zp.is_contiguous());
  TORCH_CHECK(qp.scalar_type() == torch::kInt32 &&
              sp.scalar_type() == torch::kFloat16 &&
              zp.scalar_type() == torch::kUInt8);
  check_shape(N, K, G);
  const int64_t n_chunks = (K + kChunk - 1) / kChunk;
  TORCH_CHECK(qp.numel() == (N / 16) * n_chunks * 64 * 4, "int4: codes size");
  TORCH_CHECK(sp.numel() == N * (K / G), "int4: scales size");
  TORCH_CHECK(zp.numel() == (N / 16) * (K / G) * 8, "int4: zeros size");
  TORCH_CHECK((uintptr_t)qp.data_ptr() % 16 == 0);
  return {reinterpret_cast<const uint4*>(qp.data_ptr()),
          reinterpret_cast<const __half*>(sp.data_ptr()),
          reinterpret_cast<const uint8_t*>(zp.data_ptr()),
          (int)N, (int)K, (int)G, (int)n_chunks};
}

}  // namespace w4a16
