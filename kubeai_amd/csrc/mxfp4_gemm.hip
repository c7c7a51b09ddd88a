// W4A8 with OCP microscaling FP4 weights (MXFP4): e2m1 codes, one E8M0 scale
// byte per (output row, block of 32 consecutive k), e4m3 activations with one
// fp32 scale per row.
//
//   mxfp4_dequant : packed weight -> bf16 [N, K]                (streaming)
//   mxfp4_gemm    : y[m, n] = bf16_rne(acc[m, n] * xs[m]), 1 <= M <= 64, with
//                   acc the fp32 sum over k of xq[m, k] * w[n, k]
//
// w[n, k] = e2m1(code[n, k]) * 2^(e[n, k / 32] - 127), e in [2, 252]: every
// nonzero weight is a normal bf16, and an e4m3 value times it is exact in
// fp32. The products are formed and summed by the matrix unit,
// v_mfma_scale_f32_16x16x128_f8f6f4: A is the weight tile (16 rows x 128 k,
// e2m1, 4 VGPRs per lane), B the activations (128 k x 16 tokens, e4m3, 8
// VGPRs). Lane (nl = lane & 15, kq = lane >> 4) of A holds row nl's 32
// consecutive k of quarter kq, code j in nibble j, and multiplies them by the
// scale byte that op_sel picks from its scale VGPR: a lane's 32 codes are one
// MX block, so that byte is the block's E8M0. An 8-bit operand is laid out
// differently: lane (nl, kq) of B holds token nl's k = 16 kq .. 16 kq + 15 in
// its first four registers and k = 64 + 16 kq .. + 15 in the other four
// (measured with one-hot operands; tests/test_mxfp4_gpu.py pins it). The
// activation side's scale is the constant 127 (1.0); xs[m] is applied at the
// end.
// D: lane (m = lane & 15, kq) holds rows n = kq * 4 + i, i.e. four
// neighbouring columns of y for token m: one 8-byte store.
//
// Packed layout (engine/quant_mxfp4.py packs it once). N is cut into tiles of
// 16 rows, K into chunks of 128, the last padded with zero codes:
//   codes  uint8 [N/16, Kc, 64, 16] : unit kq * 16 + nl is the 16 bytes of row
//          tile * 16 + nl from k = chunk * 128 + kq * 32, low nibble = even k
//   scales uint8 [N/16, J, 8, 64, 4]: word (j, w, lane), byte c is the scale
//          of the lane's unit in chunk 32 * j + 8 * c + w (127 where there is
//          no such chunk), J = ceil(ceil(Kc / 8) / 4)
// A workgroup of 8 waves owns 16 * NT columns over all of K; wave w takes
// chunks w, w + 8, ..., so four consecutive chunks of its walk share one scale
// word and the byte index is the unrolled loop's position, a compile-time
// op_sel. Its code loads are 1 KB contiguous per (tile, chunk), its x loads
// two 16 B per lane and row tile (two runs of 64 B per row and wave), straight
// from the e4m3 rows: nothing is staged in LDS.
//
// The waves' partial tiles are summed through LDS in wave order: one launch,
// no atomics, no workspace, and for one output the same sequence of
// operations whatever M, MT, NT and the other rows are.
#include <torch/extension.h>

#include <tuple>

#include "mxfp4_common.h"

namespace {

// kWaves, kChunk, SCALAR_F32, static_for, the MFMA wrapper and check_packed
// are shared with mxfp4_gemm_tiled.hip
using namespace mxfp4;

// chunks of codes in flight per lane and column tile (the ring is
// kAhead * NT 16-byte loads); chosen from the resource report,
// profiles/r14_mxfp4.md
template <int NT>
constexpr int kAhead = NT == 1 ? 8 : NT == 2 ? 4 : 2;

// bf16 bits of e2m1 code c (sign, 2 exponent bits, 1 mantissa bit) times
// 2^(e - 127), e in [2, 252]
DEV_INLINE uint32_t e2m1_to_bf16(const uint32_t c, const uint32_t e) {
  const uint32_t mag = c & 7u, sign = (c & 8u) << 12;
  if (mag == 0) return sign;
  if (mag == 1) return sign | ((e - 1) << 7);  // 0.5, the one subnormal
  return sign | ((e + (mag >> 1) - 1) << 7) | ((mag & 1u) << 6);
}

// One thread per 16 B unit. Lanes are mapped (nl = lane / 4, kq = lane % 4)
// so that 4 neighbouring lanes write 256 contiguous bytes of one output row.
SCALAR_F32 __launch_bounds__(256) __global__ void mxfp4_dequant_kernel(
    ushort* __restrict__ out,  // [N, K] bf16
    const uint4* __restrict__ qp, const uint8_t* __restrict__ sp, const int N,
    const int K, const int n_chunks, const int n_groups) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)(N / 16) * n_chunks * 64;
  if (u >= total) return;
  const int lane = (int)(u & 63);
  const int64_t tc = u >> 6;  // tile * n_chunks + chunk
  const int64_t tile = tc / n_chunks;
  const int chunk = (int)(tc % n_chunks);
  const int nl = lane >> 2, kq = lane & 3;
  const int k0 = chunk * kChunk + kq * 32;
  if (k0 >= K) return;  // zero padding of the last chunk
  const int unit = kq * 16 + nl;
  const uint4 c = qp[tc * 64 + unit];
  const int64_t word =
      ((tile * n_groups + chunk / 32) * kWaves + chunk % kWaves) * 64 + unit;
  const uint32_t e = sp[word * 4 + (chunk % 32) / kWaves];
  ushort* dst = out + (tile * 16 + nl) * (int64_t)K + k0;
  const uint32_t words[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    uint4 o;
    uint32_t* op = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
    for (int p = 0; p < 4; ++p)
      op[p] = e2m1_to_bf16(words[t] >> (8 * p), e) |
              (e2m1_to_bf16(words[t] >> (8 * p + 4), e) << 16);
    *reinterpret_cast<uint4*>(dst + 8 * t) = o;
  }
}

// MT: 16-row tiles of x. NT: 16-column tiles of W per workgroup.
template <int MT, int NT>
SCALAR_F32 __launch_bounds__(kWaves * WAVE_SIZE) __global__ void mxfp4_gemm_kernel(
    ushort* __restrict__ y,          // [M, N] bf16, contiguous
    const uint8_t* __restrict__ xq,  // [M, K] e4m3, row stride x_stride
    const int64_t x_stride, const float* __restrict__ xs,  // [M]
    const uint4* __restrict__ qp, const uint32_t* __restrict__ sp, const int M,
    const int N, const int K, const int n_chunks, const int n_groups) {
  constexpr int kRing = kAhead<NT>;
  constexpr int kUnroll = kRing > 4 ? kRing : 4;
  static_assert(kUnroll % 4 == 0 && kUnroll % kRing == 0);
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
  const uint8_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
    xrow[mt] = xq + (int64_t)min(mt * 16 + nl, M - 1) * x_stride;

  // This wave's i-th chunk is wave + i * kWaves. Codes run kRing chunks ahead
  // in a register ring, the scale word of iterations 4j .. 4j + 3 one word
  // ahead, the x fragments one chunk ahead in a double buffer. No load is
  // conditional: a prefetch past the wave's last chunk reads that last chunk
  // (or the last scale word) again and is never used. A load under a branch
  // lands in a temporary and is copied, and the copy made every step wait for
  // every load in flight: 6x the time (profiles/r14_mxfp4.md). The MFMA needs
  // the whole wave, so a lane in the padding of the last chunk (k >= K) stays
  // in: its codes are the packed zeros, and each half of its x fragment past
  // K is the row's k = 0 .. 15 (in bounds). Zero times those is zero unless
  // one is NaN, and then the row's sum is NaN with or without the padding.
  const int n_iter = (n_chunks - wave + kWaves - 1) / kWaves;
  const int last_chunk = wave + (max(n_iter, 1) - 1) * kWaves;
  uint4 ring[kRing][NT];
  uint32_t sw[NT], sw_next[NT];
  uint4 xb[2][MT][2];

  auto fetch_codes = [&](const int i, const int slot) __attribute__((always_inline)) {
    const int chunk = min(wave + i * kWaves, min(last_chunk, n_chunks - 1));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      ring[slot][nt] = qp[((int64_t)(tile0 + nt) * n_chunks + chunk) * 64 + lane];
  };
  auto fetch_scales = [&](const int j) __attribute__((always_inline)) {
    const int jc = min(j, n_groups - 1);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      sw_next[nt] =
          sp[(((int64_t)(tile0 + nt) * n_groups + jc) * kWaves + wave) * 64 + lane];
  };
  // half h of the lane's B fragment is x[chunk * 128 + 64 h + 16 kq ..+15]
  auto fetch_x = [&](const int i, const int buf) __attribute__((always_inline)) {
    const int chunk = min(wave + i * kWaves, min(last_chunk, n_chunks - 1));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k_lane = chunk * kChunk + 64 * h + 16 * kq;
      const int k0 = k_lane < K ? k_lane : 0;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        xb[buf][mt][h] = *reinterpret_cast<const uint4*>(xrow[mt] + k0);
    }
  };

  static_for<kRing>([&](auto uu) __attribute__((always_inline)) { fetch_codes(uu.value, uu.value); });
  fetch_scales(0);
  fetch_x(0, 0);
  // unrolled by kUnroll: ring slot, x buffer and scale byte of each step are
  // static
  for (int i0 = 0; i0 < n_iter; i0 += kUnroll) {
    static_for<kUnroll>([&](auto uu) __attribute__((always_inline)) {
      constexpr int u = decltype(uu)::value;
      constexpr int slot = u % kRing;
      const int i = i0 + u;
      if (i >= n_iter) return;
      if constexpr (u % 4 == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) sw[nt] = sw_next[nt];
        fetch_scales(i / 4 + 1);
      }
      fetch_x(i + 1, (u + 1) & 1);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const uint4 x0 = xb[u & 1][mt][0], x1 = xb[u & 1][mt][1];
        const i32x8 b = {(int)x0.x, (int)x0.y, (int)x0.z, (int)x0.w,
                         (int)x1.x, (int)x1.y, (int)x1.z, (int)x1.w};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          // e2m1 reads the first four registers only
          const uint4 c = ring[slot][nt];
          const i32x8 a = {(int)c.x, (int)c.y, (int)c.z, (int)c.w, 0, 0, 0, 0};
          acc[nt][mt] = mfma_w4a8_sel<u % 4>(a, b, acc[nt][mt], (int)sw[nt]);
        }
      }
      fetch_codes(i + kRing, slot);  // the slot this step has just read
    });
  }

  // K-split reduction, one column tile at a time through the same LDS: every
  // wave parks its partial tiles, then wave mt sums row tile mt's kWaves
  // partials in wave order and stores it.
  __shared__ f32x4 part[kWaves][MT][WAVE_SIZE];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (nt > 0) __syncthreads();  // the previous tile's partials are consumed
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) part[wave][mt][lane] = acc[nt][mt];
    __syncthreads();
    if (wave < MT) {
      f32x4 sum = part[0][wave][lane];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        const f32x4 p = part[w][wave][lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] += p[i];
      }
      const int m = wave * 16 + nl;
      if (m < M) {
        const float s = xs[m];
        uint2 o;
        o.x = f32_to_bf16(sum[0] * s) | ((uint32_t)f32_to_bf16(sum[1] * s) << 16);
        o.y = f32_to_bf16(sum[2] * s) | ((uint32_t)f32_to_bf16(sum[3] * s) << 16);
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + (tile0 + nt) * 16 +
                                  kq * 4) = o;
      }
    }
  }
}

// Column tiles (of 16) per workgroup. int4_gemm's rule (int4_gemm_tiles) and
// its reasoning: a wider workgroup reads x from L2 once for more columns, but
// owns them over all of K, so width is only taken while enough workgroups
// remain (256, or 160 above one row tile). int4's two exceptions are gone,
// from the sweep in profiles/r14_mxfp4.md: 4 x 4 tiles fit the register file
// here and win at M = 64 wherever 160 workgroups remain, and a single row
// gains from the wider workgroup on the same terms as 16 rows do.
int plan_tiles(const int64_t N, const int64_t M) {
  const int64_t kMinWorkgroups = M <= 16 ? 256 : 160;
  const int64_t tiles = N / 16;
  if (tiles % 4 == 0 && tiles / 4 >= kMinWorkgroups) return 4;
  if (tiles % 2 == 0 && tiles / 2 >= kMinWorkgroups) return 2;
  return 1;
}

}  // namespace

std::tuple<int64_t, int64_t> mxfp4_plan(int64_t M, int64_t N) {
  TORCH_CHECK(M >= 1 && M <= 64, "mxfp4_gemm supports M in [1, 64], got ", M);
  TORCH_CHECK(N > 0 && N % 16 == 0, "mxfp4: N must be a multiple of 16");
  return {(M + 15) / 16, plan_tiles(N, M)};
}

void mxfp4_dequant(torch::Tensor out, torch::Tensor qp, torch::Tensor sp,
                   int64_t N, int64_t K) {
  const Packed p = check_packed(qp, sp, N, K);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == torch::kBFloat16 &&
                  out.device() == qp.device(),
              "mxfp4_dequant: out is contiguous bf16 on the weight's GPU");
  TORCH_CHECK(out.numel() == N * K, "mxfp4_dequant: out must hold N*K bf16");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 16 == 0);
  const int64_t total = (int64_t)(p.N / 16) * p.n_chunks * 64;
  TORCH_CHECK((total + 255) / 256 < (int64_t(1) << 31));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(mxfp4_dequant_kernel,
                     dim3((uint32_t)((total + 255) / 256)), dim3(256), 0,
                     stream, (ushort*)out.data_ptr(), p.qp, p.sp, p.N, p.K,
                     p.n_chunks, p.n_groups);
  HIP_CHECK_KERNEL();
}

// n_tiles = 0 takes mxfp4_plan's column tiles per workgroup
void mxfp4_gemm(torch::Tensor y, torch::Tensor xq, torch::Tensor xs,
                torch::Tensor qp, torch::Tensor sp, int64_t N, int64_t K,
                int64_t n_tiles) {
  const Packed p = check_packed(qp, sp, N, K);
  TORCH_CHECK(xq.is_cuda() && xq.dim() == 2 &&
                  xq.scalar_type() == torch::kFloat8_e4m3fn,
              "mxfp4_gemm: xq is e4m3fn [M, K]");
  const int64_t M = xq.size(0);
  TORCH_CHECK(M >= 1 && M <= 64, "mxfp4_gemm supports M in [1, 64], got ", M);
  TORCH_CHECK(xq.size(1) == K && xq.stride(1) == 1,
              "mxfp4_gemm: xq is [M, ", K, "], got [M, ", xq.size(1), "]");
  TORCH_CHECK(xq.stride(0) >= K && xq.stride(0) % 16 == 0 &&
                  (uintptr_t)xq.data_ptr() % 16 == 0,
              "mxfp4_gemm: xq rows must be 16-byte aligned");
  TORCH_CHECK(xs.is_cuda() && xs.is_contiguous() &&
                  xs.scalar_type() == torch::kFloat32 && xs.size(0) == M &&
                  (xs.dim() == 1 || (xs.dim() == 2 && xs.size(1) == 1)),
              "mxfp4_gemm: xs is fp32 [M] or [M, 1], contiguous");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() &&
                  y.scalar_type() == torch::kBFloat16 && y.dim() == 2 &&
                  y.size(0) == M && y.size(1) == N &&
                  (uintptr_t)y.data_ptr() % 8 == 0,
              "mxfp4_gemm: y is bf16 [M, N], contiguous");
  TORCH_CHECK(xq.device() == y.device() && xq.device() == xs.device() &&
                  xq.device() == qp.device(),
              "mxfp4_gemm: all tensors must be on one device");
  if (n_tiles == 0) n_tiles = plan_tiles(N, M);
  TORCH_CHECK((n_tiles == 1 || n_tiles == 2 || n_tiles == 4) &&
                  (N / 16) % n_tiles == 0,
              "mxfp4_gemm: ", n_tiles,
              " column tiles: need 1, 2 or 4, dividing N / 16");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 3, 4>((int)(M + 15) / 16, "mxfp4_gemm M tiles", [&](auto mt) {
    dispatch_int<1, 2, 4>((int)n_tiles, "mxfp4_gemm N tiles", [&](auto nt) {
      constexpr int MT = decltype(mt)::value;
      constexpr int NT = decltype(nt)::value;
      hipLaunchKernelGGL((mxfp4_gemm_kernel<MT, NT>),
                         dim3((uint32_t)(p.N / (16 * NT))),
                         dim3(kWaves * WAVE_SIZE), 0, stream,
                         (ushort*)y.data_ptr(), (const uint8_t*)xq.data_ptr(),
                         xq.stride(0), (const float*)xs.data_ptr(), p.qp,
                         reinterpret_cast<const uint32_t*>(p.sp), (int)M, p.N,
                         p.K, p.n_chunks, p.n_groups);
    });
  });
  HIP_CHECK_KERNEL();
}
