// W4A8 MXFP4 GEMM for steps of more than 64 rows: an output-tiled kernel on
// the scaled MFMA, over the packed Mxfp4Weight exactly as mxfp4_gemm.hip reads
// it (that file's header describes the packed layout and the operand layouts
// of v_mfma_scale_f32_16x16x128_f8f6f4).
//
//   mxfp4_gemm_tiled : y[m, n] = bf16_rne(acc[m, n] * xs[m]), any M >= 1, with
//                      acc the fp32 sum over k of xq[m, k] * w[n, k]
//
// Work split. One workgroup of 4 waves computes a BM x BN tile of y over all of
// K; the grid is (ceil(N / BN), ceil(M / BM)). The waves stand 2 x 2 over the
// tile: wave (wm, wn) = (wave >> 1, wave & 1) owns rows wm * BM/2 .. and
// columns wn * BN/2 .., that is RT = BM/32 row tiles x CT = BN/32 column tiles
// of 16 x 16 accumulators. Per chunk of 128 k it loads CT weight fragments
// (one 16 B global load per lane and column tile: a (tile, chunk) of codes is
// 1 KB already in A-fragment lane order) and CT scale words, reads RT
// activation fragments from LDS and issues RT * CT MFMAs. Every output has one
// accumulator that walks all of K in the order below: no split-K, no atomics,
// no workspace. The bytes of a row of y are a function of that row of x, the
// weight and K alone, whatever M, the tile form and the other rows are. They
// are not mxfp4_gemm's bytes, which is the sum of eight wave partials; on
// exactly representable data both equal the oracle.
//
// Walk order. The scale word (j, w, unit) carries in byte c the scale of chunk
// 32 j + 8 c + w, so K is walked for j, for w, for c, skipping every chunk
// >= n_chunks: next_chunk() below. Four consecutive steps then read the four
// bytes of one word. The word is fetched again with each step's codes (4 B
// beside 16 B, from the same 256 B line the step before touched) and shifted
// right by 8 c, so the MFMA always selects byte 0: the loop body is one
// straight line for every chunk, with no branch on c and no load under a
// branch. The order depends on K alone.
//
// LDS map. The x tile of a chunk is BM rows x 128 B of e4m3, shared by the two
// waves of a tile row. Thread t stages, per pass p < BM/32, the 16 B slot
// s = t & 7 of row r = 32 p + (t >> 3) at
//     x_off(r, s) = r * 128 + ((s ^ ((r >> 1) & 7)) << 4).
// The B fragment of lane (nl, kq) of row tile i is slot kq (k = 16 kq ..) and
// slot 4 + kq (k = 64 + 16 kq ..) of row r = 16 i + nl, read through the same
// x_off: staging and read-back agree because both go through this one map of
// (row, slot), and a slot is the unit of both. Conflicts: rows 2 q and 2 q + 1
// share one 256 B span of the 64 banks. A ds_read_b128 is served 16 lanes at
// a time; those are 16 consecutive rows reading one slot s. Row parity picks
// the half of the span, and s ^ ((r >> 1) & 7) sends the 8 rows of one parity
// to 8 different slots, so the 16 lanes cover the 16 slots of a span exactly
// once. A staging write's 16 lanes are rows 2 q, 2 q + 1 x 8 slots: a
// permutation of one span under the same map.
//
// Pipeline. Two LDS buffers, one barrier per chunk, register rings of kDepth
// slots. In step t a wave
//   1. writes the x registers of its ring slot (chunk t + 1, loaded kDepth
//      steps ago) to buffer (t + 1) & 1,
//   2. reads chunk t's fragments from buffer t & 1, refills the slot with
//      chunk t + 1 + kDepth's x slots and issues the MFMAs,
//   3. refills the slot's codes and scale words with chunk t + kDepth's,
//   4. waits at the barrier.
// Buffer (t + 1) & 1 was last read in step t - 1, before that step's barrier,
// and is read next in step t + 1, after this step's: one barrier is enough.
// Every prefetch is unconditional: past the last chunk
// next_chunk() stays where it is and the loads read that chunk again. A slot
// of the last chunk's padding (k >= K) reads the row's k = 0 .. 15 instead (in
// bounds) against the packed zero codes, as in mxfp4_gemm. Rows past M read
// row M - 1 and column tiles past N read the last tile; neither is stored.
//
// Resources, the sweep behind tiled_plan() and what was tried:
// docs/kernels.md and profiles/r18_mxfp4_tiled.md.
#include <torch/extension.h>

#include <tuple>

#include "mxfp4_common.h"

namespace {

using namespace mxfp4;

constexpr int kTiledWaves = 4;
// steps between the issue of a global load and its use: the depth of the
// register rings (profiles/r18_mxfp4_tiled.md)
constexpr int kDepth = 2;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// __syncthreads() for LDS traffic, spelled with builtins. The library function
// is not inlined into a SCALAR_F32 kernel (its target features differ), and a
// call in the chunk loop spills what is live across it. The fences order LDS
// accesses only: the global prefetches stay in flight across the barrier.
DEV_INLINE void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The chunk after `chunk` in the walk for j, for w, for c over
// chunk = 32 j + 8 c + w < n_chunks; the last chunk is followed by itself.
DEV_INLINE int next_chunk(const int chunk, const int n_chunks) {
  if (((chunk >> 3) & 3) < 3 && chunk + 8 < n_chunks) return chunk + 8;
  const int j = chunk >> 5, w = chunk & 7;
  // (j, w + 1, 0), or (j + 1, 0, 0) after w = 7; where that is past the end,
  // so is everything after it
  const int next = w < 7 ? 32 * j + w + 1 : 32 * (j + 1);
  return next < n_chunks ? next : chunk;
}

template <int BM, int BN>
SCALAR_F32 __launch_bounds__(kTiledWaves * WAVE_SIZE) __global__
void mxfp4_gemm_tiled_kernel(
    ushort* __restrict__ y,          // [M, N] bf16, contiguous
    const uint8_t* __restrict__ xq,  // [M, K] e4m3, row stride x_stride
    const int64_t x_stride, const float* __restrict__ xs,  // [M]
    const uint4* __restrict__ qp, const uint32_t* __restrict__ sp, const int M,
    const int N, const int K, const int n_chunks, const int n_groups) {
  constexpr int RT = BM / 32, CT = BN / 32;  // tiles per wave
  constexpr int XP = BM / 32;                // staging passes of 32 rows
  constexpr int kBuf = BM * kChunk;          // bytes of one x tile
  __shared__ __attribute__((aligned(16))) uint8_t x_lds[2 * kBuf];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE_SIZE);
  const int lane = tid % WAVE_SIZE;
  const int nl = lane & 15, kq = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM;
  const int tile0 = blockIdx.x * (BN / 16) + wn * CT;
  const int n_tiles = N / 16;

  // staging: this thread's slot and its rows
  const int st_slot = tid & 7;
  const uint8_t* xrow[XP];
#pragma unroll
  for (int p = 0; p < XP; ++p)
    xrow[p] = xq + (int64_t)min(m0 + 32 * p + (tid >> 3), M - 1) * x_stride;
  const int st_off = (tid >> 3) * kChunk + ((st_slot ^ ((tid >> 4) & 7)) << 4);
  // read-back: slots kq and 4 + kq of row 16 i + nl; (row >> 1) & 7 = nl >> 1
  const int rd_row = (wm * (BM / 2) + nl) * kChunk;
  const int rd_off0 = rd_row + ((kq ^ (nl >> 1)) << 4);
  const int rd_off1 = rd_row + (((4 + kq) ^ (nl >> 1)) << 4);

  const uint4* wbase[CT];
  const uint32_t* sbase[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int64_t tile = min(tile0 + ct, n_tiles - 1);
    wbase[ct] = qp + tile * n_chunks * 64 + lane;
    sbase[ct] = sp + tile * n_groups * (kWaves * 64) + lane;
  }

  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = {0.f, 0.f, 0.f, 0.f};

  // Register rings, slot = step % kDepth, indexed by static_for so that they
  // stay registers. xr holds native vectors: a uint4 (a struct) copied whole
  // from a register array to LDS kept the array in scratch.
  u32x4 xr[kDepth][XP];
  uint4 wr[kDepth][CT];
  uint32_t sr[kDepth][CT];
  auto fetch_x = [&](auto slot, const int chunk) __attribute__((always_inline)) {
    const int k = chunk * kChunk + 16 * st_slot;
    const int k0 = k < K ? k : 0;
    static_for<XP>([&](auto p) __attribute__((always_inline)) {
      xr[slot.value][p.value] =
          *reinterpret_cast<const u32x4*>(xrow[p.value] + k0);
    });
  };
  auto stage_x = [&](auto slot, const int buf) __attribute__((always_inline)) {
    static_for<XP>([&](auto p) __attribute__((always_inline)) {
      *reinterpret_cast<u32x4*>(x_lds + buf * kBuf + p.value * (32 * kChunk) +
                                st_off) = xr[slot.value][p.value];
    });
  };
  auto fetch_w = [&](auto slot, const int chunk) __attribute__((always_inline)) {
    const int word = ((chunk >> 5) * kWaves + (chunk & 7)) * 64;
    static_for<CT>([&](auto ct) __attribute__((always_inline)) {
      wr[slot.value][ct.value] = wbase[ct.value][(int64_t)chunk * 64];
      sr[slot.value][ct.value] = sbase[ct.value][word];
    });
  };

  // Step t works on chunk `cur`; its slot of the rings holds the codes of
  // `cur` and the x slots of the chunk after it, and is refilled with the
  // codes of chunk t + kDepth (`cw`) and the x slots of chunk t + kDepth + 1
  // (`cx`).
  int cur = 0, cw = 0, cx = next_chunk(0, n_chunks);
  fetch_x(Int<0>{}, 0);
  stage_x(Int<0>{}, 0);
  static_for<kDepth>([&](auto u) __attribute__((always_inline)) {
    fetch_w(u, cw);
    fetch_x(u, cx);
    cw = cx;
    cx = next_chunk(cx, n_chunks);
  });
  lds_barrier();

  // unrolled by kDepth: the ring slot of each step is static. A step past the
  // last chunk (n_chunks % kDepth != 0) keeps its loads, which read the last
  // chunk again, and its barrier, and skips the MFMAs.
  for (int t0 = 0; t0 < n_chunks; t0 += kDepth) {
    static_for<kDepth>([&](auto u) __attribute__((always_inline)) {
      const int t = t0 + u.value;
      const int buf = t & 1;
      const int shift = ((cur >> 3) & 3) * 8;  // byte c of the scale word
      stage_x(u, buf ^ 1);
      const uint8_t* xt = x_lds + buf * kBuf;
      i32x8 b[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const u32x4 x0 =
            *reinterpret_cast<const u32x4*>(xt + rt * (16 * kChunk) + rd_off0);
        const u32x4 x1 =
            *reinterpret_cast<const u32x4*>(xt + rt * (16 * kChunk) + rd_off1);
        b[rt] = {(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w,
                 (int)x1.x, (int)x1.y, (int)x1.z, (int)x1.w};
      }
      fetch_x(u, cx);
      if (t < n_chunks) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          // e2m1 reads the first four registers only
          const uint4 c = wr[u.value][ct];
          const i32x8 a = {(int)c.x, (int)c.y, (int)c.z, (int)c.w, 0, 0, 0, 0};
          const int scale = (int)(sr[u.value][ct] >> shift);
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt][ct] = mfma_w4a8_sel<0>(a, b[rt], acc[rt][ct], scale);
        }
      }
      fetch_w(u, cw);  // the slot this step has just read
      lds_barrier();
      cur = next_chunk(cur, n_chunks);
      cw = cx;
      cx = next_chunk(cx, n_chunks);
    });
  }

  // D: lane (m = nl, kq) holds columns kq * 4 + i of its token: one 8 B store
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int m = m0 + wm * (BM / 2) + rt * 16 + nl;
    if (m >= M) continue;
    const float s = xs[m];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (tile0 + ct >= n_tiles) continue;
      const f32x4 v = acc[rt][ct];
      uint2 o;
      o.x = f32_to_bf16(v[0] * s) | ((uint32_t)f32_to_bf16(v[1] * s) << 16);
      o.y = f32_to_bf16(v[2] * s) | ((uint32_t)f32_to_bf16(v[3] * s) << 16);
      *reinterpret_cast<uint2*>(y + (int64_t)m * N + (tile0 + ct) * 16 +
                                kq * 4) = o;
    }
  }
}

// 64 x 128 where it still fills the chip, 64 x 64 below. A CU holds two
// 64 x 128 workgroups (2 waves per SIMD), 512 on an MI355X; in the sweep of
// profiles/r18_mxfp4_tiled.md the wide form won from 448 workgroups up (8B and
// 70B gate_up at M = 65) and lost at every count below. 128 x 128 was
// instantiated and swept too: at one wave per SIMD it lost to 64 x 128 in
// every cell, so no plan picks it and it is not built.
std::pair<int, int> tiled_plan(const int64_t M, const int64_t N) {
  constexpr int64_t kMinWorkgroups = 448;
  if (((M + 63) / 64) * ((N + 127) / 128) >= kMinWorkgroups) return {64, 128};
  return {64, 64};
}

}  // namespace

std::tuple<int64_t, int64_t> mxfp4_tiled_plan(int64_t M, int64_t N) {
  TORCH_CHECK(M >= 1, "mxfp4_gemm_tiled needs M >= 1, got ", M);
  TORCH_CHECK(N > 0 && N % 16 == 0, "mxfp4: N must be a multiple of 16");
  const auto [bm, bn] = tiled_plan(M, N);
  return {bm, bn};
}

// bm = bn = 0 takes mxfp4_tiled_plan's tile form
void mxfp4_gemm_tiled(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                      torch::Tensor qp, torch::Tensor sp, int64_t N, int64_t K,
                      int64_t bm, int64_t bn) {
  const Packed p = check_packed(qp, sp, N, K);
  TORCH_CHECK(xq.is_cuda() && xq.dim() == 2 &&
                  xq.scalar_type() == torch::kFloat8_e4m3fn,
              "mxfp4_gemm_tiled: xq is e4m3fn [M, K]");
  const int64_t M = xq.size(0);
  TORCH_CHECK(M >= 1 && M < (int64_t(1) << 31),
              "mxfp4_gemm_tiled needs M >= 1, got ", M);
  TORCH_CHECK(xq.size(1) == K && xq.stride(1) == 1,
              "mxfp4_gemm_tiled: xq is [M, ", K, "], got [M, ", xq.size(1), "]");
  TORCH_CHECK(xq.stride(0) >= K && xq.stride(0) % 16 == 0 &&
                  (uintptr_t)xq.data_ptr() % 16 == 0,
              "mxfp4_gemm_tiled: xq rows must be 16-byte aligned");
  TORCH_CHECK(xs.is_cuda() && xs.is_contiguous() &&
                  xs.scalar_type() == torch::kFloat32 && xs.size(0) == M &&
                  (xs.dim() == 1 || (xs.dim() == 2 && xs.size(1) == 1)),
              "mxfp4_gemm_tiled: xs is fp32 [M] or [M, 1], contiguous");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
                  y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
                  y.size(0) == M && y.size(1) == N &&
                  (uintptr_t)y.data_ptr() % 8 == 0,
              "mxfp4_gemm_tiled: y is bf16 [M, N], contiguous");
  TORCH_CHECK(xq.device() == y.device() && xq.device() == xs.device() &&
                  xq.device() == qp.device(),
              "mxfp4_gemm_tiled: all tensors must be on one device");
  TORCH_CHECK((bm == 0) == (bn == 0),
              "mxfp4_gemm_tiled: give both bm and bn, or neither");
  if (bm == 0) std::tie(bm, bn) = tiled_plan(M, N);
  TORCH_CHECK(bm == 64 && (bn == 128 || bn == 64),
              "mxfp4_gemm_tiled: no tile form ", bm, " x ", bn,
              " (64 x 128, 64 x 64)");
  const int64_t gx = (N + bn - 1) / bn, gy = (M + bm - 1) / bm;
  TORCH_CHECK(gy <= 65535 && gx < (int64_t(1) << 31),
              "mxfp4_gemm_tiled: grid ", gx, " x ", gy, " exceeds the limits");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  // the form is one value: 1000 * bm + bn
  dispatch_int<64128, 64064>(
      (int)(1000 * bm + bn), "mxfp4_gemm_tiled form", [&](auto form) {
        constexpr int BM = decltype(form)::value / 1000;
        constexpr int BN = decltype(form)::value % 1000;
        hipLaunchKernelGGL((mxfp4_gemm_tiled_kernel<BM, BN>),
                           dim3((uint32_t)gx, (uint32_t)gy),
                           dim3(kTiledWaves * WAVE_SIZE), 0, stream,
                           (ushort*)y.data_ptr(), (const uint8_t*)xq.data_ptr(),
                           xq.stride(0), (const float*)xs.data_ptr(), p.qp,
                           reinterpret_cast<const uint32_t*>(p.sp), (int)M, p.N,
                           p.K, p.n_chunks, p.n_groups);
      });
  HIP_CHECK_KERNEL();
}
