// W4A16 (AWQ-style asymmetric int4, fp16 group scales) kernels.
//
//   int4_dequant : packed weight -> bf16 [N, K]              (streaming)
//   int4_gemm    : y[M,N] = x[M,K] @ dequant(W)[N,K]^T, M <= 64 (fused)
//
// The pinned dequantization is w[n,k] = bf16_rne(float(q - z) * float(s)) in
// fp32. (q - z) has at most 5 significant bits and an fp16 scale 11, so the
// product is exact in fp32 and the bf16 rounding is the only rounding: both
// kernels reproduce Int4Weight.dequant() bit for bit.
//
// Packed layout (engine/quant_int4.py packs it once, at construction). N is
// cut into tiles of 16 rows, K into chunks of 128 (the last chunk zero-padded):
//   codes  int32 [N/16, Kc, 64, 4] : unit (kq, nl) = kq*16 + nl is 16 bytes,
//          the 32 consecutive-k codes of row tile*16 + nl starting at
//          k0 = chunk*128 + kq*32; code j sits in word j/8, bits 4*(j%8)..+3
//   scales fp16  [N/16, G, 16]     : group gi of the tile's 16 rows
//   zeros  uint8 [N/16, G, 8]      : row nl in byte nl/2, bits 4*(nl%2)..+3
// A wave's code load for one (tile, chunk) is 1 KB contiguous, one 16 B load
// per lane, and a wave walking K walks all three arrays contiguously.
//
// Fused GEMM. MFMA v_mfma_f32_16x16x32_bf16 sums over its 32 k-slots; which
// real k sits in which slot is free as long as A and B agree. Lane
// (nl = lane & 15, kq = lane >> 4) owns the 32 codes of unit (kq, nl); MFMA
// step t (0..3) of a chunk takes codes 8t..8t+7 of every lane, i.e. slot
// 8*kq + j holds k = chunk*128 + kq*32 + 8t + j. The matching A fragment of
// lane (m = lane & 15, kq) is x[m][that k], one 16 B load. A lane's 32 codes
// lie in one quantization group (g is a multiple of 32), so it needs one
// scale and one zero per chunk.
//
// A workgroup owns 16, 32 or 64 output columns (int4_gemm_tiles) over ALL of
// K. Its waves take chunks w, w + W, ... and their fp32 partials are summed
// through LDS in wave order: one launch, no cross-workgroup traffic, no
// atomics, no workspace, and the same bits on every run. The chunk loop and
// the reduction live in int4_common.h, shared with the grouped MoE kernel.
#include <torch/extension.h>

#include "common.h"
#include "dispatch.h"
#include "int4_common.h"

using namespace w4a16;

namespace {

// One thread per 16 B unit. Lanes are mapped (nl = lane / 4, kq = lane % 4)
// so that 4 neighbouring lanes write 256 contiguous bytes of one output row.
template <int G>
__launch_bounds__(256) __global__ void int4_dequant_kernel(
    ushort* __restrict__ out,          // [N, K] bf16
    const uint4* __restrict__ qp, const __half* __restrict__ sp,
    const uint8_t* __restrict__ zp, const int N, const int K,
    const int n_chunks) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)(N / 16) * n_chunks * 64;
  if (u >= total) return;
  const int lane = (int)(u & 63);
  const int64_t tc = u >> 6;            // tile * n_chunks + chunk
  const int64_t tile = tc / n_chunks;
  const int chunk = (int)(tc % n_chunks);
  const int nl = lane >> 2, kq = lane & 3;
  const int k0 = chunk * kChunk + kq * 32;
  if (k0 >= K) return;                  // zero padding of the last chunk
  const uint4 c = qp[tc * 64 + kq * 16 + nl];
  float s, zf;
  load_scale_zero(sp, zp, tile, K / G, k0 / G, nl, s, zf);
  ushort* dst = out + (tile * 16 + nl) * (int64_t)K + k0;
  const uint32_t words[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *reinterpret_cast<bf16x8*>(dst + 8 * t) = dequant8(words[t], zf, s);
}

// rows 0 .. M-1 of the workgroup's tiles are rows 0 .. M-1 of y
struct FirstRows {
  int M;
  DEV_INLINE bool stored(const int r) const { return r < M; }
  DEV_INLINE int row(const int r) const { return r; }
};

// MT: 16-row tiles of x. NT: 16-column tiles of W per workgroup. The chunk
// loop and the K-split reduction are int4_common.h's, shared with the
// grouped MoE kernel (int4_moe.hip).
template <int MT, int NT, int G>
__launch_bounds__(kWaves * WAVE_SIZE) __global__ void int4_gemm_kernel(
    ushort* __restrict__ y,            // [M, N] bf16, contiguous
    const ushort* __restrict__ x,      // [M, K] bf16, row stride x_stride
    const int64_t x_stride, const uint4* __restrict__ qp,
    const __half* __restrict__ sp, const uint8_t* __restrict__ zp,
    const int M, const int N, const int K, const int n_chunks) {
  const int tile0 = blockIdx.x * NT;
  // wave-uniform by construction; say so, and its branches become scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int lane = threadIdx.x % WAVE_SIZE;
  const int nl = lane & 15, kq = lane >> 4;

  f32x4 acc[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = {0.f, 0.f, 0.f, 0.f};

  // rows past M read row M-1 (in bounds, never stored)
  const ushort* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] = x + (int64_t)min(mt * 16 + nl, M - 1) * x_stride;

  int4_chunk_loop<MT, MT, NT, G>(acc, xrow, qp, sp, zp, tile0, K, n_chunks,
                                 wave, lane, nl, kq);

  __shared__ float part[kWaves][MT][4][WAVE_SIZE];
  int4_reduce_store<MT, NT>(y, acc, part, N, tile0, wave, lane, nl, kq,
                            FirstRows{M});
}

}  // namespace

// Column tiles (of 16) per workgroup of the fused kernel. Every workgroup reads
// all of x from L2, M * K * 2 bytes against its 8 * K * NT bytes of codes, so
// wider workgroups cut that traffic; but a workgroup owns its columns over all
// of K, so width is only taken while enough workgroups remain to fill the
// GPU: one per CU of an MI355X up to one row tile, 160 above it, where the x
// traffic weighs more (measured: 160 and 192 workgroups gain, 128 lose;
// profiles/r07_int4.md). A single row (M == 1) is a broadcast load and stays
// at 1; 4 row tiles by 4 column tiles would not fit the register file
// without scratch and is not instantiated.
int64_t int4_gemm_tiles(int64_t N, int64_t M) {
  const int64_t kMinWorkgroups = M <= 16 ? 256 : 160;
  const int64_t tiles = N / 16;
  if (M <= 1) return 1;
  if (M <= 48 && tiles % 4 == 0 && tiles / 4 >= kMinWorkgroups) return 4;
  if (tiles % 2 == 0 && tiles / 2 >= kMinWorkgroups) return 2;
  return 1;
}

void int4_dequant(torch::Tensor out, torch::Tensor qp, torch::Tensor sp,
                  torch::Tensor zp, int64_t N, int64_t K, int64_t group) {
  const Packed p = check_packed(qp, sp, zp, N, K, group);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
              out.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(out.numel() == N * K, "int4_dequant: out must hold N*K bf16");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0);
  const int64_t total = (int64_t)(p.N / 16) * p.n_chunks * 64;
  TORCH_CHECK((total + 255) / 256 < (int64_t(1) << 31));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<32, 64, 128>(p.G, "int4 group size", [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((int4_dequant_kernel<G>),
                       dim3((uint32_t)((total + 255) / 256)), dim3(256), 0,
                       stream, (ushort*)out.data_ptr(), p.qp, p.sp, p.zp, p.N,
                       p.K, p.n_chunks);
  });
  HIP_CHECK_KERNEL();
}

void int4_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor qp,
               torch::Tensor sp, torch::Tensor zp, int64_t N, int64_t K,
               int64_t group) {
  const Packed p = check_packed(qp, sp, zp, N, K, group);
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.size(1) == K && x.stride(1) == 1, "int4_gemm: x is [M, K]");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= 64, "int4_gemm supports M in [1, 64]");
  TORCH_CHECK(x.stride(0) >= K && x.stride(0) % 8 == 0 &&
                  (uintptr_t)x.data_ptr() % 16 == 0,
              "int4_gemm: x rows must be 16-byte aligned");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
              y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
              y.size(0) == M && y.size(1) == N);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int n_tiles = int4_gemm_tiles(p.N, (int)M);
  dispatch_int<1, 2, 3, 4>((int)(M + 15) / 16, "int4_gemm M tiles", [&](auto mt) {
    dispatch_int<1, 2, 4>(n_tiles, "int4_gemm N tiles", [&](auto nt) {
      dispatch_int<32, 64, 128>(p.G, "int4 group size", [&](auto g) {
        constexpr int MT = decltype(mt)::value;
        constexpr int NT = decltype(nt)::value;
        constexpr int G = decltype(g)::value;
        if constexpr (MT * NT < 16)
          hipLaunchKernelGGL((int4_gemm_kernel<MT, NT, G>),
                             dim3(p.N / (16 * NT)), dim3(kWaves * WAVE_SIZE),
                             0, stream, (ushort*)y.data_ptr(),
                             (const ushort*)x.data_ptr(), x.stride(0), p.qp,
                             p.sp, p.zp, (int)M, p.N, p.K, p.n_chunks);
        else
          TORCH_CHECK(false, "int4_gemm: no 4 x 4 tile kernel");
      });
    });
  });
  HIP_CHECK_KERNEL();
}
