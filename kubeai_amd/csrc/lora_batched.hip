// Batched multi-LoRA apply for decode steps (T <= 64), routed on the device:
// every adapter of the batch in two launches, static shapes, graph-safe.
//
//   y[t, :] = bf16(float(y[t, :]) + B_s . vb[t, :])      s = slots[t] >= 1
//   vb[t, r] = bf16(scale_s * sum_k A_s[r, k] * x[t, k])
//
// Rows with slot 0 (base model, pad rows) and rows whose slot has R == 0 are
// never written. The design is the grouped MoE GEMMs' (fp8_moe.hip): a device
// table of weight addresses written when an adapter is loaded, the routing
// (`slots`, int32 [T]) read by the kernels, a row list per workgroup in LDS
// (moe_routing.h), an early return where a slot has no row, a K split that is
// reduced in a fixed order. No atomics, nothing between the workgroups of a
// launch, and no workspace that grows: `vpart` is allocated by the caller.
//
// Table: int64 [S, 4] per (target, layer), row s = (address of A_s [R, K],
// address of B_s [N, R], R, scale as fp32 bits); row 0 is not read. The grids
// have S - 1 in y whatever adapters the batch names.
//
// lora_shrink, grid (KS, S - 1): vpart[ks, t, r] = sum over the k of split ks
// of A_s[r, k] * x[t, k] in fp32, [KS, T, 64]. v_mfma_f32_16x16x32_bf16 with
// the listed tokens as rows and the ranks as columns: lane (nl = lane & 15,
// kq = lane >> 4) feeds the 16 bytes at k = chunk * 32 + kq * 8 of x row
// list[mt * 16 + nl] and of A row rt * 16 + nl, so both operands put the same
// k into the same k-slot. A lane past K, or whose rank is >= R, supplies
// zeros and does not load. Split ks owns chunks [ks * per, (ks + 1) * per),
// wave w of 8 takes every 8th of them from the w-th on, in order; the 8
// partial tiles are added in wave order through LDS. lora_expand then adds
// the splits in ascending ks: the order of the whole fp32 sum is a function
// of K and KS alone, so a row has the same bits whatever else is in the
// batch, from run to run and under graph replay.
//
// lora_expand, grid (ceil(N / 128), S - 1), one 16-column tile per wave: the
// workgroup forms vb for its rows once in LDS (the one rounding the per-token
// sgmv kernel does not have: it keeps v in fp32), then each wave runs 1-2
// MFMA k-steps (k = rank) per token tile with B_s[n, 0:R] as it lies. The
// weight columns are the MFMA's rows here, so a lane ends up with 4
// neighbouring columns of one token's row and updates y with 8-byte accesses.
#include <torch/extension.h>

#include <tuple>

#include "common.h"
#include "dispatch.h"
#include "moe_routing.h"

// v_pk_*_f32 stay out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

using moe::kMaxRows;
using moe::kWaves;

namespace {

constexpr int kStep = 32;        // k per MFMA
constexpr int kMaxRank = 64;     // 4 rank tiles; row stride of vpart
constexpr int kRankTiles = kMaxRank / 16;
constexpr int kMaxSplits = 32;   // K splits of lora_shrink
constexpr int kVbStride = kMaxRank + 8;  // LDS row of vb, padded off the banks

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;  // one 16 B load

DEV_INLINE f32x4 mfma_bf16(const u32x4 a, const u32x4 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

DEV_INLINE u32x4 load16_if(const bool live, const ushort* p) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if (live) v = *reinterpret_cast<const u32x4*>(p);
  return v;
}

struct Slot {
  const ushort* A;
  const ushort* B;
  int R;
  float scale;
};

DEV_INLINE Slot read_slot(const int64_t* __restrict__ table, const int slot) {
  const int64_t* e = table + (int64_t)slot * 4;
  Slot s;
  s.A = reinterpret_cast<const ushort*>(e[0]);
  s.B = reinterpret_cast<const ushort*>(e[1]);
  s.R = (int)e[2];
  s.scale = __builtin_bit_cast(float, (uint32_t)e[3]);
  return s;
}

// acc[rt][mt] += x rows of tile mt times ranks of tile rt over this wave's
// chunks of [c_begin, c_end). LT row tiles and RT rank tiles are live.
template <int MT, int LT, int RT>
DEV_INLINE void shrink_loop(f32x4 (&acc)[kRankTiles][MT],
                            const ushort* (&xrow)[MT],
                            const ushort* (&arow)[kRankTiles],
                            const bool (&rank_live)[kRankTiles], const int K,
                            const int c_begin, const int c_end, const int wave,
                            const int kq) {
  for (int c = c_begin + wave; c < c_end; c += kWaves) {
    const int k = c * kStep + kq * 8;
    const bool in_k = k < K;
    u32x4 xa[LT], aa[RT];
#pragma unroll
    for (int mt = 0; mt < LT; ++mt) xa[mt] = load16_if(in_k, xrow[mt] + k);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      aa[rt] = load16_if(in_k && rank_live[rt], arow[rt] + k);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int mt = 0; mt < LT; ++mt)
        acc[rt][mt] = mfma_bf16(xa[mt], aa[rt], acc[rt][mt]);
  }
}

template <int MT>
__launch_bounds__(kWaves * WAVE_SIZE) __global__ void lora_shrink_kernel(
    float* __restrict__ vpart,         // [KS, T, kMaxRank]
    const ushort* __restrict__ x,      // [T, K] bf16, row stride
    const int64_t x_stride,
    const int* __restrict__ slots,     // [T]
    const int T,
    const int64_t* __restrict__ table, // [S, 4]
    const int K, const int n_chunks, const int per_split) {
  const int ks = blockIdx.x;
  const int slot = blockIdx.y + 1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int lane = threadIdx.x % WAVE_SIZE;
  const int nl = lane & 15, kq = lane >> 4;

  // the rows of this slot, in ascending row order (moe_routing.h)
  __shared__ int list[kMaxRows];
  __shared__ int wave_hits[kWaves];
  const int count =
      moe::build_pair_list(list, wave_hits, slots, T, slot, wave, lane);
  if (count == 0) return;  // the whole workgroup: no weight is touched
  const Slot s = read_slot(table, slot);
  if (s.R <= 0 || s.R > kMaxRank || (s.R & 7)) return;  // nothing to add
  __syncthreads();

  f32x4 acc[kRankTiles][MT];
#pragma unroll
  for (int rt = 0; rt < kRankTiles; ++rt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[rt][mt] = {0.f, 0.f, 0.f, 0.f};

  // rows past the count read the last listed row (in bounds, never stored);
  // ranks past R read nothing (the pointer stays inside A all the same)
  const ushort* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] = x + (int64_t)list[min(mt * 16 + nl, count - 1)] * x_stride;
  const ushort* arow[kRankTiles];
  bool rank_live[kRankTiles];
#pragma unroll
  for (int rt = 0; rt < kRankTiles; ++rt) {
    const int r = rt * 16 + nl;
    rank_live[rt] = r < s.R;
    arow[rt] = s.A + (int64_t)min(r, s.R - 1) * K;
  }

  const int c_begin = min(ks * per_split, n_chunks);
  const int c_end = min(c_begin + per_split, n_chunks);
  const int live = (count + 15) / 16;
  const int n_rt = (s.R + 15) / 16;
  moe::dispatch_live<MT>(live, [&](auto lt) {
    moe::dispatch_live<kRankTiles>(n_rt, [&](auto rtiles) {
      shrink_loop<MT, decltype(lt)::value, decltype(rtiles)::value>(
          acc, xrow, arow, rank_live, K, c_begin, c_end, wave, kq);
    });
  });

  // The waves' partial tiles, one rank tile at a time through the same LDS:
  // the MT * 4 accumulator registers are dealt out to the waves and each lane
  // sums its register's kWaves partials in wave order.
  // C layout: lane holds rows (lane >> 4) * 4 + i, column lane & 15.
  __shared__ float part[kWaves][MT][4][WAVE_SIZE];
#pragma unroll
  for (int rt = 0; rt < kRankTiles; ++rt) {
    if (rt < n_rt) {  // uniform over the workgroup
      if (rt > 0) __syncthreads();  // the previous tile's partials are consumed
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][mt][i][lane] = acc[rt][mt][i];
      __syncthreads();
      for (int e = wave; e < MT * 4; e += kWaves) {
        const int mt = e >> 2, i = e & 3;
        const int row = mt * 16 + kq * 4 + i;
        if (row >= count) continue;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += part[w][mt][i][lane];
        vpart[((int64_t)ks * T + list[row]) * kMaxRank + rt * 16 + nl] = sum;
      }
    }
  }
}

template <int MT>
__launch_bounds__(kWaves * WAVE_SIZE) __global__ void lora_expand_kernel(
    ushort* __restrict__ y,            // [T, N] bf16, row stride (+=)
    const int64_t y_stride,
    const float* __restrict__ vpart,   // [KS, T, kMaxRank]
    const int* __restrict__ slots,     // [T]
    const int T,
    const int64_t* __restrict__ table, // [S, 4]
    const int N, const int KS) {
  const int slot = blockIdx.y + 1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int lane = threadIdx.x % WAVE_SIZE;
  const int nl = lane & 15, kq = lane >> 4;

  __shared__ int list[kMaxRows];
  __shared__ int wave_hits[kWaves];
  const int count =
      moe::build_pair_list(list, wave_hits, slots, T, slot, wave, lane);
  if (count == 0) return;
  const Slot s = read_slot(table, slot);
  if (s.R <= 0 || s.R > kMaxRank || (s.R & 7)) return;
  __syncthreads();

  // vb[row, r] = bf16(scale * sum_ks vpart[ks, list[row], r]), ks ascending:
  // thread u owns 8 ranks of one row (count * R / 8 <= 512 units)
  __shared__ __attribute__((aligned(16))) ushort vb[kMaxRows][kVbStride];
  {
    const int r8 = s.R / 8;
    const int row = threadIdx.x / r8, rg = threadIdx.x % r8;
    if (row < count) {
      const float* p = vpart + (int64_t)list[row] * kMaxRank + rg * 8;
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < KS; ++ks) {
        const float* q = p + (int64_t)ks * T * kMaxRank;
        lo += *reinterpret_cast<const f32x4*>(q);
        hi += *reinterpret_cast<const f32x4*>(q + 4);
      }
      ushort8 out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[j] = f32_to_bf16(s.scale * lo[j]);
        out[4 + j] = f32_to_bf16(s.scale * hi[j]);
      }
      *reinterpret_cast<ushort8*>(&vb[row][rg * 8]) = out;
    }
  }
  __syncthreads();

  // no barrier below: a wave whose column tile is past N leaves
  const int col0 = (blockIdx.x * kWaves + wave) * 16;
  if (col0 >= N) return;

  // MFMA rows are the weight's columns col0 + nl, MFMA columns the tokens:
  // lane (nl, kq) ends with y[list[mt * 16 + nl], col0 + kq * 4 + 0..3]
  const int live = (count + 15) / 16;
  const ushort* brow = s.B + (int64_t)(col0 + nl) * s.R;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int step = 0; step < kMaxRank / kStep; ++step) {
    if (step * kStep < s.R) {  // wave-uniform
      const int r0 = step * kStep + kq * 8;
      const bool in_r = r0 < s.R;
      const u32x4 b = load16_if(in_r, brow + r0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (mt < live) {  // wave-uniform
          const int row = mt * 16 + nl;
          const u32x4 a = load16_if(in_r && row < count, &vb[row][r0]);
          acc[mt] = mfma_bf16(b, a, acc[mt]);
        }
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = mt * 16 + nl;
    if (mt < live && row < count) {
      ushort4_t* yp = reinterpret_cast<ushort4_t*>(
          y + (int64_t)list[row] * y_stride + col0 + kq * 4);
      ushort4_t v = *yp;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = f32_to_bf16(bf16_to_f32(v[i]) + acc[mt][i]);
      *yp = v;
    }
  }
}

}  // namespace

#pragma clang attribute pop

// K splits of lora_shrink. One adapter's rows are served by KS workgroups,
// and a workgroup streams its share of A (R x K bf16) and of the rows of x;
// every split costs each lora_expand workgroup one more [rows, R] fp32 read.
// A split gets kChunksPerSplit chunks of 32 k (two per wave), up to
// kPlanSplits splits. From the sweep over KS = 1 .. 32 in
// profiles/r12_lora.md (one apply under graph replay, rank 16 and 64, T = 8
// and 64, 1 and 4 adapters): at K = 4096 KS = 8 is the fastest or within
// 0.4 us of it (KS = 1: up to 2.3 times slower); at K = 14336 KS = 16 is the
// fastest or within 1.1 us of it (KS = 1: up to 4.9 times slower), and
// KS = 32 is 2 .. 4 us slower again at every point.
constexpr int kChunksPerSplit = 16;
constexpr int kPlanSplits = 16;

int64_t lora_splits(int64_t K) {
  const int64_t n_chunks = (K + kStep - 1) / kStep;
  const int64_t ks = (n_chunks + kChunksPerSplit - 1) / kChunksPerSplit;
  return std::max<int64_t>(1, std::min<int64_t>(ks, kPlanSplits));
}

std::tuple<int64_t, int64_t> lora_plan(int64_t T, int64_t K) {
  TORCH_CHECK(T >= 1 && T <= kMaxRows && K > 0 && K % 8 == 0,
              "lora_plan: need 1 <= T <= 64 and K % 8 == 0");
  return {(T + 15) / 16, lora_splits(K)};
}

void lora_apply(torch::Tensor y, torch::Tensor x, torch::Tensor slots,
                torch::Tensor table, torch::Tensor table_host,
                torch::Tensor vpart, int64_t ks) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
                  x.scalar_type() == torch::kBFloat16 && x.stride(1) == 1,
              "lora_apply: x is bf16 [T, K] with unit inner stride");
  TORCH_CHECK(y.is_cuda() && y.dim() == 2 &&
                  y.scalar_type() == torch::kBFloat16 && y.stride(1) == 1,
              "lora_apply: y is bf16 [T, N] with unit inner stride");
  const int64_t T = x.size(0), K = x.size(1), N = y.size(1);
  TORCH_CHECK(T >= 1 && T <= kMaxRows, "lora_apply supports T in [1, 64], got ",
              T);
  TORCH_CHECK(y.size(0) == T, "lora_apply: y has ", y.size(0), " rows, x ", T);
  TORCH_CHECK(K > 0 && K % 8 == 0, "lora_apply: K must be a multiple of 8, got ",
              K);
  TORCH_CHECK(N > 0 && N % 16 == 0,
              "lora_apply: N must be a multiple of 16, got ", N);
  TORCH_CHECK(K < (int64_t(1) << 30) && N < (int64_t(1) << 30));
  TORCH_CHECK(x.stride(0) >= K && x.stride(0) % 8 == 0 &&
                  (uintptr_t)x.data_ptr() % 16 == 0,
              "lora_apply: x rows must be 16-byte aligned");
  TORCH_CHECK(y.stride(0) >= N && y.stride(0) % 4 == 0 &&
                  (uintptr_t)y.data_ptr() % 8 == 0,
              "lora_apply: y rows must be 8-byte aligned");
  TORCH_CHECK(slots.is_cuda() && slots.dim() == 1 && slots.size(0) == T &&
                  slots.is_contiguous() &&
                  slots.scalar_type() == torch::kInt32,
              "lora_apply: slots is int32 [T], contiguous");
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
                  table.scalar_type() == torch::kInt64 && table.dim() == 2 &&
                  table.size(0) >= 2 && table.size(0) <= 256 &&
                  table.size(1) == 4,
              "lora_apply: table is int64 [S, 4], 2 <= S <= 256");
  const int64_t S = table.size(0);
  // the rows are checked on the host copy the table's owner keeps: reading
  // the device table here would be a sync, and one inside a graph capture
  TORCH_CHECK(!table_host.is_cuda() && table_host.is_contiguous() &&
                  table_host.scalar_type() == torch::kInt64 &&
                  table_host.sizes() == table.sizes(),
              "lora_apply: table_host is the table's host copy");
  const int64_t* rows = table_host.data_ptr<int64_t>();
  for (int64_t s = 1; s < S; ++s) {
    const int64_t R = rows[s * 4 + 2];
    TORCH_CHECK(R >= 0 && R <= kMaxRank && R % 8 == 0, "lora_apply: slot ", s,
                " has rank ", R, ", need a multiple of 8 up to 64");
    TORCH_CHECK(R == 0 || (rows[s * 4] != 0 && rows[s * 4] % 16 == 0 &&
                           rows[s * 4 + 1] != 0 && rows[s * 4 + 1] % 16 == 0),
                "lora_apply: slot ", s, ": A and B must be 16-byte aligned");
  }
  if (ks == 0) ks = lora_splits(K);
  TORCH_CHECK(ks >= 1 && ks <= kMaxSplits, "lora_apply: ", ks,
              " K splits, need 1 .. ", kMaxSplits);
  TORCH_CHECK(vpart.is_cuda() && vpart.is_contiguous() &&
                  vpart.scalar_type() == torch::kFloat32 &&
                  vpart.numel() >= ks * T * kMaxRank &&
                  (uintptr_t)vpart.data_ptr() % 16 == 0,
              "lora_apply: vpart is fp32 with at least KS * T * 64 elements");
  TORCH_CHECK(x.device() == y.device() && x.device() == slots.device() &&
                  x.device() == table.device() && x.device() == vpart.device(),
              "lora_apply: all tensors must be on one device");

  const int n_chunks = (int)((K + kStep - 1) / kStep);
  const int per_split = (int)((n_chunks + ks - 1) / ks);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 3, 4>((int)(T + 15) / 16, "lora_apply M tiles", [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    hipLaunchKernelGGL((lora_shrink_kernel<MT>),
                       dim3((uint32_t)ks, (uint32_t)(S - 1)),
                       dim3(kWaves * WAVE_SIZE), 0, stream,
                       (float*)vpart.data_ptr(), (const ushort*)x.data_ptr(),
                       x.stride(0), (const int*)slots.data_ptr(), (int)T,
                       (const int64_t*)table.data_ptr(), (int)K, n_chunks,
                       per_split);
    hipLaunchKernelGGL((lora_expand_kernel<MT>),
                       dim3((uint32_t)((N + 16 * kWaves - 1) / (16 * kWaves)),
                            (uint32_t)(S - 1)),
                       dim3(kWaves * WAVE_SIZE), 0, stream,
                       (ushort*)y.data_ptr(), y.stride(0),
                       (const float*)vpart.data_ptr(),
                       (const int*)slots.data_ptr(), (int)T,
                       (const int64_t*)table.data_ptr(), (int)N, (int)ks);
  });
  HIP_CHECK_KERNEL();
}
