// Grouped fp8 (W8A8, e4m3fn) expert GEMMs for MoE decode, routed on the
// device: the fp8 sibling of int4_moe_gemm (int4_moe.hip).
//
//   fp8_moe_gemm : y[p, n] = bf16((acc * xs[r]) * ws_e[n]),
//                  acc = sum_k float(xq[r, k]) * float(wq_e[n, k]) in fp32,
//                  for every pair p = t * k + j with e = selected[t, j] and
//                  r = p / row_div; one launch for all E experts of one
//                  projection
//
// This is Fp8Linear.forward_quantized for that row and expert up to the order
// of the fp32 sum (every e4m3 x e4m3 product is exact in fp32). The kernel
// fixes the order as a function of K alone, so a row of y has the same bits
// whatever else is in the batch, whatever T, MT or NT serve it, from run to
// run and under graph replay.
//
// Workgroup (column block, e) lists the pairs routed to expert e in LDS
// (moe_routing.h), takes its lanes' x rows and its tiles' y rows from that
// list and streams its columns of expert e's weight once, as it lies in
// memory ([N, K] row-major e4m3, no repacking). An expert with no pair
// returns before it reads any weight or scale, so only the routed experts'
// weights cross HBM. No atomics, no workspace, no traffic between workgroups.
//
// MFMA: v_mfma_f32_16x16x32_fp8_fp8, 8 bytes of A (x) and 8 of B (w) per
// lane. Lane (nl = lane & 15, kq = lane >> 4) holds row nl of the x tile and
// row tile * 16 + nl of the weight; of a 128-wide chunk of K it reads the 32
// bytes at k = chunk * 128 + kq * 32 of both (two 16 B loads; four lanes
// cover one 128 B line of a row) and feeds MFMA t = 0..3 bytes 8t .. 8t+7 of
// each. Which real k lands in which of the instruction's 32 k-slots is then
// the same for A and B, and that is all the product needs
// (tests/test_fp8_moe_gpu.py checks the map with exact integer data).
//
// K split: wave w of 8 takes chunks w, w + 8, ... in order, four MFMAs per
// chunk in order of t; the 8 partial tiles are added in wave order through
// LDS. K must be a multiple of 32, so that a lane's 32 bytes are wholly
// inside a row or wholly in the zero padding of the last chunk.
#include <torch/extension.h>

#include <cmath>
#include <tuple>

#include "common.h"
#include "dispatch.h"
#include "moe_routing.h"

using moe::kMaxRows;
using moe::kMaxTopK;
using moe::kWaves;

namespace {

constexpr int kChunk = 128;   // k (= bytes of a row) per (wave, iteration)
constexpr int kRing = 4;      // weight fetches (chunk x column tile) in flight

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) long i64x2;  // one 16 B load

// The chunk loop of one workgroup: acc[nt][mt] += x rows of tile mt times
// column tile tile0 + nt, over this wave's chunks wave, wave + kWaves, ...
// MT, LT and NT as in int4_chunk_loop (int4_common.h), and the same two-stage
// software pipeline: the weight bytes of all NT tiles are fetched kAhead
// chunks ahead into a register ring (kAhead * NT = kRing fetches of 32 B in
// flight per lane), the x fragments one chunk ahead into the other half of a
// double buffer. All guards on `chunk < n_chunks` are wave-uniform. A lane in
// the zero padding of the last chunk (k >= K) stays in with zero A and B
// fragments; it reads k = 0, which is in bounds.
template <int MT, int LT, int NT>
DEV_INLINE void fp8_chunk_loop(f32x4 (&acc)[NT][MT],
                               const uint8_t* (&xrow)[MT],
                               const uint8_t* __restrict__ wq, const int tile0,
                               const int K, const int n_chunks, const int wave,
                               const int nl, const int kq) {
  constexpr int kAhead = kRing / NT;
  i64x2 ring[kAhead][NT][2];
  i64x2 a[2][LT][2];

  const uint8_t* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    wrow[nt] = wq + (int64_t)((tile0 + nt) * 16 + nl) * K;

  auto lane_k = [&](const int chunk, bool& live) {
    const int k_lane = chunk * kChunk + kq * 32;
    live = k_lane < K;
    return live ? k_lane : 0;
  };
  auto fetch_w = [&](const int i, const int slot) {
    const int chunk = wave + i * kWaves;
    if (chunk >= n_chunks) return;
    bool live;
    const int k0 = lane_k(chunk, live);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ring[slot][nt][h] =
            *reinterpret_cast<const i64x2*>(wrow[nt] + k0 + 16 * h);
        if (!live) ring[slot][nt][h] = i64x2{0, 0};
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
      for (int h = 0; h < 2; ++h) {
        a[buf][mt][h] = *reinterpret_cast<const i64x2*>(xrow[mt] + k0 + 16 * h);
        if (!live) a[buf][mt][h] = i64x2{0, 0};
      }
  };

#pragma unroll
  for (int u = 0; u < kAhead; ++u) fetch_w(u, u);
  fetch_x(0, 0);
  const int n_iter = (n_chunks - wave + kWaves - 1) / kWaves;
  // unrolled by 2 * kAhead: ring slot and x buffer of each step are static
  for (int i0 = 0; i0 < n_iter; i0 += 2 * kAhead) {
#pragma unroll
    for (int u = 0; u < 2 * kAhead; ++u) {
      const int i = i0 + u;
      if (i < n_iter) {
        const int slot = u % kAhead;
        i64x2 b[NT][2];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int h = 0; h < 2; ++h) b[nt][h] = ring[slot][nt][h];
        fetch_x(i + 1, (u + 1) & 1);
        fetch_w(i + kAhead, slot);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int mt = 0; mt < LT; ++mt)
              acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                  a[u & 1][mt][t >> 1][t & 1], b[nt][t >> 1][t & 1],
                  acc[nt][mt], 0, 0, 0);
      }
    }
  }
}

// bf16, round to nearest even: v_cvt_pk_bf16_f32
DEV_INLINE ushort cvt_bf16(const float v) {
  const f32x2 pair = {v, 0.f};
  const uint32_t packed =
      __builtin_bit_cast(uint32_t, __builtin_convertvector(pair, bf16x2));
  return (ushort)(packed & 0xffffu);
}

template <int MT, int NT>
__launch_bounds__(kWaves * WAVE_SIZE) __global__ void fp8_moe_gemm_kernel(
    ushort* __restrict__ y,            // [n_pairs, N] bf16, contiguous
    const uint8_t* __restrict__ xq,    // [n_pairs / row_div, K] e4m3, row stride
    const int64_t x_stride,
    const float* __restrict__ xs,      // [n_pairs / row_div] row scales
    const int64_t* __restrict__ selected,  // [n_pairs] expert id of pair p
    const int n_pairs, const int row_div,
    const int64_t* __restrict__ table,     // [E, 2] weight, scale addresses
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

  const int64_t* entry = table + (int64_t)expert * 2;
  const uint8_t* __restrict__ wq = reinterpret_cast<const uint8_t*>(entry[0]);
  const float* __restrict__ ws = reinterpret_cast<const float*>(entry[1]);

  f32x4 acc[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = {0.f, 0.f, 0.f, 0.f};

  // rows past the count read the last listed row (in bounds, never stored)
  const uint8_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] =
        xq + (int64_t)(list[min(mt * 16 + nl, count - 1)] / row_div) * x_stride;

  // Row tiles past the count load no x and issue no MFMA: the loop is
  // entered with the number of tiles that have rows, one wave-uniform branch
  // for the whole of K.
  const int live = (count + 15) / 16;
  moe::dispatch_live<MT>(live, [&](auto lt) {
    constexpr int LT = decltype(lt)::value;
    fp8_chunk_loop<MT, LT, NT>(acc, xrow, wq, tile0, K, n_chunks, wave, nl, kq);
  });

  // K-split reduction as in int4_reduce_store, one column tile at a time
  // through the same LDS: every wave parks its partial tile; the MT * 4
  // accumulator registers are dealt out to the waves, and each lane sums its
  // register's kWaves partials in wave order, applies the row's and then the
  // column's scale (two roundings, as written: there is nothing to contract)
  // and stores where the row is a listed pair.
  // C layout: lane holds rows (lane >> 4) * 4 + i, column lane & 15.
  __shared__ float part[kWaves][MT][4][WAVE_SIZE];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (nt > 0) __syncthreads();  // the previous tile's partials are consumed
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[wave][mt][i][lane] = acc[nt][mt][i];
    __syncthreads();
    const int col = (tile0 + nt) * 16 + nl;
    for (int e = wave; e < MT * 4; e += kWaves) {
      const int mt = e >> 2, i = e & 3;
      const int row = mt * 16 + kq * 4 + i;
      if (row >= count) continue;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += part[w][mt][i][lane];
      const int pair = list[row];
      const float scaled = (sum * xs[pair / row_div]) * ws[col];
      y[(int64_t)pair * N + col] = cvt_bf16(scaled);
    }
  }
}

}  // namespace

// Column tiles (of 16) per workgroup of fp8_moe_gemm: int4_moe_tiles' rule
// (int4_moe.hip). The host plans for uniform routing, under which
// E * (1 - (1 - k/E)^T) experts are expected to be active; a workgroup owns
// its columns over all of K, so width is taken only while the active experts
// still launch kMinWorkgroups workgroups. Measured on the 8x7B shapes
// (profiles/r11_fp8_moe.md): on down (K = 14336) wider workgroups lost where
// they left 256 and 352 expected workgroups (T = 1: 24 -> 34 us, T = 4:
// 56 -> 72 us) and gained at 448 (T = 2: 51 -> 45 us) and 461, so the floor
// sits between; gate_up is within 6% across widths up to T = 16. 4 row tiles
// by 4 column tiles is not instantiated.
int64_t fp8_moe_tiles(int64_t N, int64_t T, int64_t E, int64_t k) {
  constexpr double kMinWorkgroups = 400.0;
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

std::tuple<int64_t, int64_t> fp8_moe_plan(int64_t N, int64_t T, int64_t E,
                                          int64_t k) {
  TORCH_CHECK(N > 0 && N % 16 == 0 && T >= 1 && T <= kMaxRows && E >= 1 &&
                  k >= 1 && k <= kMaxTopK,
              "fp8_moe_plan: need N % 16 == 0, 1 <= T <= 64, 1 <= k <= 8");
  return {(T + 15) / 16, fp8_moe_tiles(N, T, E, k)};
}

void fp8_moe_gemm(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                  torch::Tensor selected, torch::Tensor table, int64_t row_div,
                  int64_t E, int64_t N, int64_t K, int64_t n_tiles) {
  TORCH_CHECK(N > 0 && N % 16 == 0, "fp8_moe_gemm: N must be a multiple of 16");
  TORCH_CHECK(K > 0 && K % 32 == 0, "fp8_moe_gemm: K must be a multiple of 32");
  TORCH_CHECK(N * K < (int64_t(1) << 40));
  TORCH_CHECK(selected.is_cuda() && selected.dim() == 2 &&
                  selected.is_contiguous() &&
                  selected.scalar_type() == torch::kInt64,
              "fp8_moe_gemm: selected is int64 [T, k], contiguous");
  const int64_t T = selected.size(0), k = selected.size(1);
  TORCH_CHECK(T >= 1 && T <= kMaxRows, "fp8_moe_gemm supports T in [1, 64]");
  TORCH_CHECK(k >= 1 && k <= kMaxTopK, "fp8_moe_gemm supports k in [1, 8]");
  const int64_t n_pairs = T * k;
  TORCH_CHECK(xq.is_cuda() && xq.dim() == 2 &&
                  xq.scalar_type() == torch::kFloat8_e4m3fn,
              "fp8_moe_gemm: xq is e4m3fn [R, K]");
  TORCH_CHECK(xq.size(1) == K && xq.stride(1) == 1,
              "fp8_moe_gemm: xq is [R, K]");
  TORCH_CHECK(xq.stride(0) >= K && xq.stride(0) % 16 == 0 &&
                  (uintptr_t)xq.data_ptr() % 16 == 0,
              "fp8_moe_gemm: xq rows must be 16-byte aligned");
  TORCH_CHECK(row_div >= 1 && xq.size(0) * row_div == n_pairs,
              "fp8_moe_gemm: xq has ", xq.size(0), " rows, need T * k / row_div"
              " = ", n_pairs, " / ", row_div);
  TORCH_CHECK(xs.is_cuda() && xs.is_contiguous() &&
                  xs.scalar_type() == torch::kFloat32 &&
                  xs.numel() == xq.size(0),
              "fp8_moe_gemm: xs is fp32, one scale per row of xq");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
                  y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
                  y.size(0) == n_pairs && y.size(1) == N,
              "fp8_moe_gemm: y is bf16 [T * k, N], contiguous");
  TORCH_CHECK(E >= 1 && E <= 65535);
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
                  table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                  table.size(0) == E && table.size(1) == 2,
              "fp8_moe_gemm: table is int64 [E, 2]");
  TORCH_CHECK(xq.device() == y.device() && xq.device() == xs.device() &&
                  xq.device() == selected.device() &&
                  xq.device() == table.device(),
              "fp8_moe_gemm: all tensors must be on one device");
  if (n_tiles == 0) n_tiles = fp8_moe_tiles(N, T, E, k);
  TORCH_CHECK((n_tiles == 1 || n_tiles == 2 || n_tiles == 4) &&
                  (N / 16) % n_tiles == 0,
              "fp8_moe_gemm: ", n_tiles,
              " column tiles: need 1, 2 or 4, dividing N / 16");
  const int n_chunks = (int)((K + kChunk - 1) / kChunk);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 3, 4>((int)(T + 15) / 16, "fp8_moe_gemm M tiles", [&](auto mt) {
    dispatch_int<1, 2, 4>((int)n_tiles, "fp8_moe_gemm N tiles", [&](auto nt) {
      constexpr int MT = decltype(mt)::value;
      constexpr int NT = decltype(nt)::value;
      if constexpr (MT * NT < 16)
        hipLaunchKernelGGL(
            (fp8_moe_gemm_kernel<MT, NT>),
            dim3((uint32_t)(N / (16 * NT)), (uint32_t)E),
            dim3(kWaves * WAVE_SIZE), 0, stream, (ushort*)y.data_ptr(),
            (const uint8_t*)xq.data_ptr(), xq.stride(0),
            (const float*)xs.data_ptr(), (const int64_t*)selected.data_ptr(),
            (int)n_pairs, (int)row_div, (const int64_t*)table.data_ptr(),
            (int)N, (int)K, n_chunks);
      else
        TORCH_CHECK(false, "fp8_moe_gemm: no 4 x 4 tile kernel");
    });
  });
  HIP_CHECK_KERNEL();
}
