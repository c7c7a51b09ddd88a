// Grouped W4A16 expert GEMMs for MoE decode, routed on the device.
//
//   int4_moe_gemm : y[p] = x[p / row_div] @ dequant(W_e)^T for every pair
//                   p = t * k + j with e = selected[t, j]; one launch for
//                   all E experts of one projection
//   moe_combine   : out[t] = sum_j w[t, j] * y[t * k + j], in the order and
//                   rounding of the dense expert loop
//
// The routing (torch.topk's int64 [T, k]) is read by the kernels, so every
// shape is static and the block captures into a graph; a replay follows
// whatever routing its buffers hold then.
//
// int4_moe_gemm_kernel is int4_gemm_kernel (int4_gemm.hip) with gathered
// rows: workgroup (column block, e) lists the pairs routed to expert e in
// LDS, takes its lanes' x rows and its tiles' y rows from that list and runs
// the shared chunk loop and reduction of int4_common.h on expert e's packed
// weight. A row's value is what int4_gemm gives for it, bit for bit. An
// expert with no pair returns before it reads any weight, scale or zero, so
// only the routed experts' weights cross HBM. No atomics, no workspace, no
// traffic between workgroups.
#include <torch/extension.h>

#include <cmath>
#include <tuple>

#include "common.h"
#include "dispatch.h"
#include "int4_common.h"
#include "moe_routing.h"

using namespace w4a16;
using moe::dispatch_live;
using moe::kMaxPairs;
using moe::kMaxRows;
using moe::kMaxTopK;
using moe::ListedRows;

namespace {

static_assert(kWaves == moe::kWaves, "the pair list is built by 8 waves");

template <int MT, int NT, int G>
__launch_bounds__(kWaves * WAVE_SIZE) __global__ void int4_moe_gemm_kernel(
    ushort* __restrict__ y,            // [n_pairs, N] bf16, contiguous
    const ushort* __restrict__ x,      // [n_pairs / row_div, K], row stride
    const int64_t x_stride,
    const int64_t* __restrict__ selected,  // [n_pairs] expert id of pair p
    const int n_pairs, const int row_div,
    const int64_t* __restrict__ table,     // [E, 3] qp, sp, zp addresses
    const int N, const int K, const int n_chunks) {
  const int tile0 = blockIdx.x * NT;
  const int expert = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int lane = threadIdx.x % WAVE_SIZE;
  const int nl = lane & 15, kq = lane >> 4;

  // the pairs of this expert, in ascending pair order (moe_routing.h)
  __shared__ int list[kMaxRows];
  __shared__ int wave_hits[kWaves];
  const int count = moe::build_pair_list(list, wave_hits, selected, n_pairs,
                                         expert, wave, lane);
  if (count == 0) return;  // the whole workgroup: no weight is touched
  __syncthreads();

  const int64_t* entry = table + (int64_t)expert * 3;
  const uint4* __restrict__ qp = reinterpret_cast<const uint4*>(entry[0]);
  const __half* __restrict__ sp = reinterpret_cast<const __half*>(entry[1]);
  const uint8_t* __restrict__ zp = reinterpret_cast<const uint8_t*>(entry[2]);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = {0.f, 0.f, 0.f, 0.f};

  // rows past the count read the last listed row (in bounds, never stored)
  const ushort* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] =
        x + (int64_t)(list[min(mt * 16 + nl, count - 1)] / row_div) * x_stride;

  // Row tiles past the count load no x and issue no MFMA: the loop is
  // entered with the number of tiles that have rows, one wave-uniform branch
  // for the whole of K.
  const int live = (count + 15) / 16;
  dispatch_live<MT>(live, [&](auto lt) {
    constexpr int LT = decltype(lt)::value;
    int4_chunk_loop<MT, LT, NT, G>(acc, xrow, qp, sp, zp, tile0, K, n_chunks,
                                   wave, lane, nl, kq);
  });

  __shared__ float part[kWaves][MT][4][WAVE_SIZE];
  int4_reduce_store<MT, NT>(y, acc, part, N, tile0, wave, lane, nl, kq,
                            ListedRows{list, count});
}

// One step of the dense loop's `out + contrib * w`: both in bf16, the
// product rounded before the sum. Contraction is pinned off, as in
// rope_rotate_pair: a fused multiply-add would skip the product's rounding.
DEV_INLINE ushort combine_term(const ushort yv, const float w) {
#pragma clang fp contract(off)
  return f32_to_bf16(bf16_to_f32(yv) * w);
}
DEV_INLINE ushort combine_add(const ushort acc, const ushort term) {
#pragma clang fp contract(off)
  return f32_to_bf16(bf16_to_f32(acc) + bf16_to_f32(term));
}

// One workgroup per token. The token's pairs are sorted by expert id in
// registers (the dense loop adds expert 0 first); ids outside [0, E) sort
// last and are skipped.
__launch_bounds__(256) __global__ void moe_combine_kernel(
    ushort* __restrict__ out,          // [T, H] bf16
    const ushort* __restrict__ y,      // [T * k, H] bf16
    const int64_t* __restrict__ selected,  // [T, k]
    const ushort* __restrict__ weights,    // [T, k] bf16
    const int k, const int H, const int E) {
  constexpr int kNone = 0x7fffffff;
  const int t = blockIdx.x;
  int key[kMaxTopK], pair[kMaxTopK];
  float w[kMaxTopK];
#pragma unroll
  for (int j = 0; j < kMaxTopK; ++j) {
    key[j] = kNone;
    pair[j] = 0;
    w[j] = 0.f;
    if (j < k) {
      const int64_t id = selected[(int64_t)t * k + j];
      if (id >= 0 && id < (int64_t)E) key[j] = (int)id;
      pair[j] = t * k + j;
      w[j] = bf16_to_f32(weights[(int64_t)t * k + j]);
    }
  }
#pragma unroll
  for (int a = 0; a < kMaxTopK - 1; ++a)
#pragma unroll
    for (int b = 0; b < kMaxTopK - 1 - a; ++b) {
      const bool swap = key[b + 1] < key[b];
      const int k0 = key[b], p0 = pair[b];
      const float w0 = w[b];
      key[b] = swap ? key[b + 1] : k0;
      pair[b] = swap ? pair[b + 1] : p0;
      w[b] = swap ? w[b + 1] : w0;
      key[b + 1] = swap ? k0 : key[b + 1];
      pair[b + 1] = swap ? p0 : pair[b + 1];
      w[b + 1] = swap ? w0 : w[b + 1];
    }

  for (int c = threadIdx.x * 8; c < H; c += blockDim.x * 8) {
    ushort8 acc = {0, 0, 0, 0, 0, 0, 0, 0};
    bool first = true;
#pragma unroll
    for (int s = 0; s < kMaxTopK; ++s) {
      if (key[s] == kNone) continue;  // same for every thread
      const ushort8 v =
          *reinterpret_cast<const ushort8*>(y + (int64_t)pair[s] * H + c);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const ushort term = combine_term(v[i], w[s]);
        acc[i] = first ? term : combine_add(acc[i], term);
      }
      first = false;
    }
    *reinterpret_cast<ushort8*>(out + (int64_t)t * H + c) = acc;
  }
}

}  // namespace

// Column tiles (of 16) per workgroup of int4_moe_gemm. The host does not know
// the routing, so it plans for uniform routing: E * (1 - (1 - k/E)^T) experts
// are expected to be active, and only their workgroups do any work. Wider
// workgroups amortise the list build, the x reads and the K-split reduction
// (gate_up, K = 4096: 66 -> 48 us at T = 1, 378 -> 207 us at T = 32), but a
// workgroup owns its columns over all of K, so width is taken only while the
// active experts still launch kMinWorkgroups workgroups. Measured on the
// 8x7B shapes (profiles/r10_int4_moe.md): 4 or 2 tiles lost where that left
// 256 and 448 expected workgroups and gained at 461 and above, so the floor
// sits between. 4 row tiles by 4 column tiles is not instantiated.
int64_t int4_moe_tiles(int64_t N, int64_t T, int64_t E, int64_t k) {
  constexpr double kMinWorkgroups = 450.0;
  const int64_t tiles = N / 16;
  const int64_t mt = (T + 15) / 16;
  const double idle = 1.0 - (double)std::min(k, E) / (double)E;
  const double active = (double)E * (1.0 - std::pow(idle, (double)T));
  for (const int64_t nt : {4, 2}) {
    if (mt * nt >= 16 || tiles % nt != 0) continue;
    if (active * (double)(tiles / nt) >= kMinWorkgroups) return nt;
  }
  return 1;
}

std::tuple<int64_t, int64_t> int4_moe_plan(int64_t N, int64_t T, int64_t E,
                                           int64_t k) {
  TORCH_CHECK(N > 0 && N % 16 == 0 && T >= 1 && T <= kMaxRows && E >= 1 &&
                  k >= 1 && k <= kMaxTopK,
              "int4_moe_plan: need N % 16 == 0, 1 <= T <= 64, 1 <= k <= 8");
  return {(T + 15) / 16, int4_moe_tiles(N, T, E, k)};
}

void int4_moe_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor selected,
                   torch::Tensor table, int64_t row_div, int64_t E, int64_t N,
                   int64_t K, int64_t group, int64_t n_tiles) {
  check_shape(N, K, group);
  TORCH_CHECK(selected.is_cuda() && selected.dim() == 2 &&
                  selected.is_contiguous() &&
                  selected.scalar_type() == torch::kInt64,
              "int4_moe_gemm: selected is int64 [T, k], contiguous");
  const int64_t T = selected.size(0), k = selected.size(1);
  TORCH_CHECK(T >= 1 && T <= kMaxRows, "int4_moe_gemm supports T in [1, 64]");
  TORCH_CHECK(k >= 1 && k <= kMaxTopK, "int4_moe_gemm supports k in [1, 8]");
  const int64_t n_pairs = T * k;
  static_assert(kMaxRows * kMaxTopK <= kMaxPairs, "one entry per thread");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.size(1) == K && x.stride(1) == 1, "int4_moe_gemm: x is [R, K]");
  TORCH_CHECK(x.stride(0) >= K && x.stride(0) % 8 == 0 &&
                  (uintptr_t)x.data_ptr() % 16 == 0,
              "int4_moe_gemm: x rows must be 16-byte aligned");
  TORCH_CHECK(row_div >= 1 && x.size(0) * row_div == n_pairs,
              "int4_moe_gemm: x has ", x.size(0), " rows, need T * k / row_div"
              " = ", n_pairs, " / ", row_div);
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
              y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
              y.size(0) == n_pairs && y.size(1) == N);
  TORCH_CHECK(E >= 1 && E <= 65535);
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
                  table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                  table.size(0) == E && table.size(1) == 3,
              "int4_moe_gemm: table is int64 [E, 3]");
  TORCH_CHECK(x.device() == y.device() && x.device() == selected.device() &&
              x.device() == table.device());
  if (n_tiles == 0) n_tiles = int4_moe_tiles(N, T, E, k);
  TORCH_CHECK((N / 16) % n_tiles == 0, "int4_moe_gemm: ", n_tiles,
              " column tiles do not divide N / 16");
  const int n_chunks = (int)((K + kChunk - 1) / kChunk);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 3, 4>((int)(T + 15) / 16, "int4_moe_gemm M tiles", [&](auto mt) {
    dispatch_int<1, 2, 4>((int)n_tiles, "int4_moe_gemm N tiles", [&](auto nt) {
      dispatch_int<32, 64, 128>((int)group, "int4 group size", [&](auto g) {
        constexpr int MT = decltype(mt)::value;
        constexpr int NT = decltype(nt)::value;
        constexpr int G = decltype(g)::value;
        if constexpr (MT * NT < 16)
          hipLaunchKernelGGL(
              (int4_moe_gemm_kernel<MT, NT, G>),
              dim3((uint32_t)(N / (16 * NT)), (uint32_t)E),
              dim3(kWaves * WAVE_SIZE), 0, stream, (ushort*)y.data_ptr(),
              (const ushort*)x.data_ptr(), x.stride(0),
              (const int64_t*)selected.data_ptr(), (int)n_pairs, (int)row_div,
              (const int64_t*)table.data_ptr(), (int)N, (int)K, n_chunks);
        else
          TORCH_CHECK(false, "int4_moe_gemm: no 4 x 4 tile kernel");
      });
    });
  });
  HIP_CHECK_KERNEL();
}

void moe_combine(torch::Tensor out, torch::Tensor y, torch::Tensor selected,
                 torch::Tensor weights, int64_t E) {
  TORCH_CHECK(selected.is_cuda() && selected.dim() == 2 &&
                  selected.is_contiguous() &&
                  selected.scalar_type() == torch::kInt64,
              "moe_combine: selected is int64 [T, k], contiguous");
  const int64_t T = selected.size(0), k = selected.size(1);
  TORCH_CHECK(T >= 1 && T < (int64_t(1) << 24) && k >= 1 && k <= kMaxTopK,
              "moe_combine supports k in [1, 8]");
  TORCH_CHECK(weights.is_cuda() && weights.is_contiguous() &&
                  weights.scalar_type() == torch::kBFloat16 &&
                  weights.dim() == 2 && weights.size(0) == T &&
                  weights.size(1) == k,
              "moe_combine: weights is bf16 [T, k], contiguous");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && y.dim() == 2 &&
              y.scalar_type() == torch::kBFloat16 && y.size(0) == T * k);
  const int64_t H = y.size(1);
  TORCH_CHECK(H > 0 && H % 8 == 0 && H < (int64_t(1) << 24),
              "moe_combine: H must be a multiple of 8");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2 &&
              out.scalar_type() == torch::kBFloat16 && out.size(0) == T &&
              out.size(1) == H);
  TORCH_CHECK((uintptr_t)y.data_ptr() % 16 == 0 &&
              (uintptr_t)out.data_ptr() % 16 == 0);
  TORCH_CHECK(y.device() == out.device() && y.device() == selected.device() &&
              y.device() == weights.device());
  // E <= 0: every non-negative id is taken
  const int e_lim = (E > 0 && E < 0x7fffffff) ? (int)E : 0x7fffffff;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(moe_combine_kernel, dim3((uint32_t)T), dim3(256), 0,
                     stream, (ushort*)out.data_ptr(),
                     (const ushort*)y.data_ptr(),
                     (const int64_t*)selected.data_ptr(),
                     (const ushort*)weights.data_ptr(), (int)k, (int)H, e_lim);
  HIP_CHECK_KERNEL();
}
