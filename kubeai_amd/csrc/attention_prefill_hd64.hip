// Paged flash-attention prefill at head_dim 64 (Llama-3.2-1B, Qwen2 /
// Qwen2.5-0.5B, TinyLlama-class models) on gfx950. One kernel for every group
// size in scope.
//
// Semantics: kubeai_amd/ops/ref.py::paged_attention_prefill. Scope: hd 64,
// causal, no window, no softcap, bf16 or e5m2 cache, G in {1, 2, 4, 7, 8}.
//
// Row map: that of attention_prefill_packed.hip. For one (sequence, kv head)
// the q_len * G (token, head) pairs are virtual rows r = t * G + g, cut into
// workgroups of 8 waves x 32 rows; row r reads q[s0 + t][kv_head * G + g],
// attends keys <= ctx + t and its softmax state is a per-lane scalar of the
// swapped product S^T = K.Q^T. G is a compile-time divisor, so G = 1, 2, 4, 8
// need no wave map of their own.
//
// What hd 64 changes against the hd-128 kernels:
//  - QK^T has 4 k-steps of v_mfma_f32_32x32x16_bf16 per 32-key subtile and O^T
//    2 accumulator tiles (32 fp32 registers instead of 64); Q is 4 B-fragments
//    (16 registers). The kernel needs no launch-bounds trick to stay out of
//    scratch.
//  - a K row is 128 B, so rows 2j and 2j + 1 share one 256 B span of the 64
//    LDS banks. The A-fragment read (ds_read_b128) has 16 lanes reading the
//    same 16 B chunk ch of 16 consecutive rows: unswizzled they fall on 2 of
//    the 16 chunk slots of the span. Row parity already picks the half of the
//    span; XORing the chunk index with (row >> 1) & 7 makes the 8 rows of one
//    parity take 8 different chunks, so the 16 lanes cover all 16 slots:
//        k_off(row, byte) = row * 128 + (byte ^ (((row >> 1) & 7) << 4)).
//    The staging writes (16 lanes = rows 2j, 2j + 1 x 8 chunks) are a
//    permutation of one span under the same map.
//  - V is stored in 4-token x 16-element subtiles (128 B, the unit
//    ds_read_b64_tr_b16 transposes), 4 subtiles across head_dim instead of 8:
//        v_off(tok, hd) = ((tok >> 2) * 4 + (hd >> 4)) * 128 B
//                         + (tok & 3) * 32 B + (hd & 15) * 2 B.
//    A PV B-fragment (V[ks * 16 + hi * 8 + jj][nb * 32 + lane % 32]) is two
//    transposed reads 512 B apart (jj < 4, jj >= 4); the 32 lanes of a half
//    read one contiguous 256 B span.
//  - a KV tile of kKVB = 64 keys is 8 KB of K and 8 KB of V: double buffered
//    32 KB, so two workgroups fit a CU where the hd-128 kernels fit one.
//
// Per tile the scheme is the packed kernel's: next tile's global loads issued
// ahead of this tile's MFMAs and written to the other buffer after them, one
// barrier per tile, P packed to bf16 in registers as the PV A-fragment,
// defer-max rescale, l summed from the unrounded fp32 p, e5m2 widened to bf16
// while staging, keys past the workgroup's causal limit never loaded and
// staged as zeros.
#include <torch/extension.h>

#include <type_traits>

#include "attention_checks.h"
#include "attention_plan.h"
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int kHD = 64;
constexpr int kBS = 16;   // cache block size (tokens)
constexpr int kKVB = 64;  // kv tokens per staged tile (a multiple of 32)
constexpr int kNSUB = kKVB / 32;  // 32-key score subtiles per tile
constexpr int kNKS = kKVB / 16;   // 16-key PV steps per tile
constexpr int kQB = 32;   // virtual rows per wave
constexpr int kNW = 8;    // waves per workgroup
constexpr int kROWS = kNW * kQB;  // virtual rows per workgroup
constexpr int kRowB = kHD * 2;    // bytes of a K row in LDS

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// byte offset of 16 B chunk `byte_off / 16` of K row `row` (derivation above)
DEV_INLINE int k_off(int row, int byte_off) {
  return row * kRowB + (byte_off ^ (((row >> 1) & 7) << 4));
}

// element offset of V[tok][hd] in the 4 x 16 subtiled layout
DEV_INLINE int v_off(int tok, int hd) {
  return ((tok >> 2) * (kHD / 16) + (hd >> 4)) * 64 + (tok & 3) * 16 +
         (hd & 15);
}

DEV_INLINE uint32_t cvt_pk_bf16(float a, float b) {
  uint32_t r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// C-fragment row of the 32x32 MFMA for register index `reg`, lane half `hi`
DEV_INLINE int crow(int reg, int hi) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * hi;
}

template <int G, typename CT>
__launch_bounds__(kNW * WAVE_SIZE) __global__ void paged_prefill_hd64_kernel(
    ushort* __restrict__ out,            // [Tq, n_q, 64]
    const ushort* __restrict__ q,        // [Tq, n_q, 64], rows q_stride apart
    const CT* __restrict__ k_cache,      // [nb, n_kv, 16, 64]
    const CT* __restrict__ v_cache,
    const int32_t* __restrict__ block_tables,     // [B, max_blocks]
    const int32_t* __restrict__ query_start_loc,  // [B+1]
    const int32_t* __restrict__ seq_lens,         // [B]
    const float scale, const int n_kv, const int max_blocks,
    const int64_t q_stride) {
  const int b = blockIdx.x;
  const int kh = blockIdx.y;
  const int n_q = n_kv * G;
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const int hi = lane >> 5;
  const int ln31 = lane & 31;

  const int s0 = query_start_loc[b];
  const int q_len = query_start_loc[b + 1] - s0;
  const int n_vrows = q_len * G;
  const int row_lo = blockIdx.z * kROWS;  // workgroup's first virtual row
  if (row_lo >= n_vrows) return;          // uniform workgroup exit
  const int ctx = seq_lens[b] - q_len;

  // keys the workgroup needs: up to the position of its last real token
  const int row_end = min(row_lo + kROWS, n_vrows);  // exclusive
  const int kv_limit = ctx + (row_end - 1) / G + 1;  // exclusive
  const int n_tiles = (kv_limit + kKVB - 1) / kKVB;

  // my wave's rows [wrow_lo, wrow_end); empty for the trailing waves of the
  // last chunk, which then only stage
  const int wrow_lo = row_lo + wave * kQB;
  const int wrow_end = min(wrow_lo + kQB, row_end);
  const bool wave_live = wrow_lo < row_end;
  const bool wave_full = wrow_lo + kQB <= row_end;
  const int wave_pos_lo = ctx + wrow_lo / G;  // position of the first row
  const int wave_pos_hi =                     // and of the last real one
      wave_live ? ctx + (wrow_end - 1) / G : -1;

  // my lane's row (the C-fragment column ln31 of the swapped product)
  const int my_row = wrow_lo + ln31;
  const bool row_ok = my_row < row_end;
  const int my_rc = min(my_row, n_vrows - 1);  // clamped for the q load
  const int my_t = my_rc / G;
  const int my_g = my_rc - my_t * G;
  const int qpos = ctx + my_t;  // last key this row may see

  __shared__ __attribute__((aligned(16))) ushort k_lds[2][kKVB * kHD];
  __shared__ __attribute__((aligned(16))) ushort v_lds[2][kKVB * kHD];

  // ---- Q in registers: B-fragment per 16-wide hd chunk ----------------
  bf16x8 q_frag[kHD / 16];
  {
    const ushort* qp = q + (int64_t)(s0 + my_t) * q_stride +
                       (int64_t)(kh * G + my_g) * kHD;
#pragma unroll
    for (int c = 0; c < kHD / 16; ++c)
      q_frag[c] = *reinterpret_cast<const bf16x8*>(qp + c * 16 + hi * 8);
  }

  f32x16 o_acc[kHD / 32];
#pragma unroll
  for (int nb = 0; nb < kHD / 32; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[nb][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int32_t* bt = block_tables + (int64_t)b * max_blocks;

  // ---- cooperative staging: 8-element units, NSTG of K and of V per thread
  // and tile; unit u: tok = u >> 3, 16 B chunk c8 = u & 7
  constexpr int NSTG = (kKVB * kHD / 8) / (kNW * WAVE_SIZE);
  static_assert(NSTG >= 1, "a tile has at least one unit per thread");
  bf16x8 st_k[NSTG], st_v[NSTG];
  bool st_ok[NSTG];
  int h_tok[NSTG], h_coff[NSTG], h_kdst[NSTG], h_vdst[NSTG];
#pragma unroll
  for (int i = 0; i < NSTG; ++i) {
    const int u = threadIdx.x + i * kNW * WAVE_SIZE;
    const int tok = u >> 3;
    const int c8 = u & 7;
    h_tok[i] = tok;
    h_coff[i] = c8 * 8;
    h_kdst[i] = k_off(tok, c8 * 16);
    h_vdst[i] = v_off(tok, c8 * 8);
  }
  auto issue_tile_loads = [&](int kt) {
    const int kv_start = kt * kKVB;
    const int kv_valid = min(kKVB, kv_limit - kv_start);
#pragma unroll
    for (int i = 0; i < NSTG; ++i) {
      st_ok[i] = h_tok[i] < kv_valid;
      if (st_ok[i]) {
        // abs_tok < kv_limit <= seq_len: inside the sequence's block table
        const int abs_tok = kv_start + h_tok[i];
        const int64_t blk = bt[abs_tok / kBS];
        const int64_t base =
            (((blk * n_kv + kh) * kBS) + abs_tok % kBS) * kHD + h_coff[i];
        if constexpr (sizeof(CT) == 2) {
          st_k[i] = *reinterpret_cast<const bf16x8*>(k_cache + base);
          st_v[i] = *reinterpret_cast<const bf16x8*>(v_cache + base);
        } else {
          // e5m2: 8-byte loads, widened to bf16 on the way into LDS
          const ushort8 kc = e5m2x8_to_bf16x8(
              *reinterpret_cast<const uint64_t*>(k_cache + base));
          const ushort8 vc = e5m2x8_to_bf16x8(
              *reinterpret_cast<const uint64_t*>(v_cache + base));
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            st_k[i][j] = (short)kc[j];
            st_v[i][j] = (short)vc[j];
          }
        }
      } else {
        // keys past the workgroup's limit: V staged as zeros (p = 0 there,
        // but 0 * stale NaN would poison the PV accumulator); K may stay
        // stale, those scores are forced to -inf
#pragma unroll
        for (int j = 0; j < 8; ++j) st_v[i][j] = 0;
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NSTG; ++i) {
      if (st_ok[i])
        *reinterpret_cast<bf16x8*>(
            reinterpret_cast<char*>(k_lds[buf]) + h_kdst[i]) = st_k[i];
      *reinterpret_cast<bf16x8*>(&v_lds[buf][h_vdst[i]]) = st_v[i];
    }
  };

  issue_tile_loads(0);
  write_tile(0);
  __syncthreads();

  for (int kt = 0; kt < n_tiles; ++kt) {
    const int cur = kt & 1;
    const int kv_start = kt * kKVB;
    const int kv_valid = min(kKVB, kv_limit - kv_start);
    const bool have_next = kt + 1 < n_tiles;
    if (have_next) issue_tile_loads(kt + 1);

    // wave-level skip: every row of this wave causally precedes the tile
    // (or the wave has no rows at all)
    if (kv_start <= wave_pos_hi) {
      // ---- S^T = K . Q^T, 4 k-steps per 32-key subtile ----------------
      __builtin_amdgcn_s_setprio(1);
      f32x16 st2[kNSUB];
#pragma unroll
      for (int sub = 0; sub < kNSUB; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st2[sub][r] = 0.f;
        const int tok = sub * 32 + ln31;
#pragma unroll
        for (int c = 0; c < kHD / 16; ++c) {
          const bf16x8 k_frag = *reinterpret_cast<const bf16x8*>(
              reinterpret_cast<const char*>(k_lds[cur]) +
              k_off(tok, c * 32 + hi * 16));
          st2[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              k_frag, q_frag[c], st2[sub], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- mask + per-lane online softmax (row = column ln31) --------
      // interior: the whole tile is visible to the wave's FIRST row, hence
      // to all of them, every staged key is real and every row is live
      const bool tile_interior = kv_valid == kKVB && wave_full &&
                                 kv_start + kKVB - 1 <= wave_pos_lo;
      float pmax = -INFINITY;
      if (tile_interior) {
#pragma unroll
        for (int sub = 0; sub < kNSUB; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float s = st2[sub][r] * scale;
            st2[sub][r] = s;
            pmax = fmaxf(pmax, s);
          }
      } else {
        // the lane's own limit ctx + r / G (qpos < kv_limit always, so the
        // staged-key bound needs no term of its own)
        const int kv_hi = row_ok ? qpos : -1;
#pragma unroll
        for (int sub = 0; sub < kNSUB; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv_start + sub * 32 + crow(r, hi);
            float s = st2[sub][r] * scale;
            if (kv > kv_hi) s = -INFINITY;
            st2[sub][r] = s;
            pmax = fmaxf(pmax, s);
          }
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));  // merge lane halves
      // defer-max: no rescale while no row's max grows by more than 8
      const bool defer = __all(pmax <= m_run + 8.f);
      float m_new = m_run;
      if (!defer) {
        m_new = fmaxf(m_run, pmax);
        const float corr =
            (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
        l_run *= corr;
        // o_acc rows are C-fragment rows crow(r, hi), not this lane's
        // softmax row: each takes the correction of its owning lane
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float cr = __shfl(corr, (lane & 32) + crow(r, hi), 64);
#pragma unroll
          for (int nb = 0; nb < kHD / 32; ++nb) o_acc[nb][r] *= cr;
        }
      }
      float rsum = 0.f;
#pragma unroll
      for (int sub = 0; sub < kNSUB; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // a row with nothing visible yet has m_new = -inf: its p is 0
          const float p = (st2[sub][r] == -INFINITY)
                              ? 0.f
                              : __expf(st2[sub][r] - m_new);
          st2[sub][r] = p;
          rsum += p;
        }
      rsum += __shfl_xor(rsum, 32, 64);
      l_run += rsum;  // from the unrounded p
      m_run = m_new;

      // ---- P -> PV A-fragments, in registers -------------------------
      // pa[ks]: lane holds P[row ln31][ks*16 + hi*8 + jj], jj = 0..7. The
      // quad jj < 4 lives in half 0's registers, jj >= 4 in half 1's; each
      // lane packs the quad its partner needs, one shfl_xor(32) swaps them.
      bf16x8 pa[kNKS];
#pragma unroll
      for (int ks = 0; ks < kNKS; ++ks) {
        const int sub = ks >> 1;
        const int q8_own = (ks & 1) * 2 + hi;
        const uint32_t own0 =
            cvt_pk_bf16(st2[sub][4 * q8_own], st2[sub][4 * q8_own + 1]);
        const uint32_t own1 =
            cvt_pk_bf16(st2[sub][4 * q8_own + 2], st2[sub][4 * q8_own + 3]);
        const int q8_par = (ks & 1) * 2 + 1 - hi;
        const uint32_t snd0 =
            cvt_pk_bf16(st2[sub][4 * q8_par], st2[sub][4 * q8_par + 1]);
        const uint32_t snd1 =
            cvt_pk_bf16(st2[sub][4 * q8_par + 2], st2[sub][4 * q8_par + 3]);
        const uint32_t got0 = __shfl_xor((int)snd0, 32, 64);
        const uint32_t got1 = __shfl_xor((int)snd1, 32, 64);
        uint32_t* pw = reinterpret_cast<uint32_t*>(&pa[ks]);
        pw[0] = hi ? got0 : own0;
        pw[1] = hi ? got1 : own1;
        pw[2] = hi ? own0 : got0;
        pw[3] = hi ? own1 : got1;
      }

      // ---- O += P.V through the hardware-transpose V read ------------
      // lane l, element jj must receive V[ks*16 + hi*8 + jj][nb*32 + ln31].
      // Within a 16-lane group the transposed read hands lane i the column i
      // of the 4 x 16 subtile whose row (i >> 2), elements 4 * (i & 3).. each
      // lane addresses. With v_off that is the byte address
      //   ks*2048 + hi*1024 + (jj>>2)*512 + nb*256 + ((l>>4)&1)*128
      //     + ((l>>2)&3)*32 + (l&3)*8
      __builtin_amdgcn_s_setprio(1);
      typedef __attribute__((address_space(3))) const char as3_char;
      as3_char* vbase =
          (as3_char*)(v_lds[cur]) +
          (hi * 1024 + ((lane >> 4) & 1) * 128 + ((lane >> 2) & 3) * 32 +
           (lane & 3) * 8);
#pragma unroll
      for (int nb = 0; nb < kHD / 32; ++nb) {
#pragma unroll
        for (int ks = 0; ks < kNKS; ++ks) {
          bf16x4 lo4, hi4;
          as3_char* a0 = vbase + ks * 2048 + nb * 256;
          // "=&v": an output aliased with the address register would let
          // the first read's writeback race the second read's address
          asm volatile(
              "ds_read_b64_tr_b16 %0, %2\n\t"
              "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
              "s_waitcnt lgkmcnt(0)"
              : "=&v"(lo4), "=&v"(hi4)
              : "v"(a0));
          bf16x8 v_frag;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v_frag[j] = lo4[j];
            v_frag[4 + j] = hi4[j];
          }
          o_acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pa[ks], v_frag, o_acc[nb], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    // one barrier per tile: the write goes to the buffer nobody reads in
    // this iteration, and the previous barrier closed its last reads
    if (have_next) write_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- normalize + write O --------------------------------------------
  // accumulator row crow(r, hi) belongs to virtual row wrow_lo + crow: its
  // 1/l comes from the lane that owns that row's softmax state, its
  // (token, head) from the row map
  const float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float inv = __shfl(inv_l, (lane & 32) + crow(r, hi), 64);
    const int vr = wrow_lo + crow(r, hi);
    if (vr >= row_end) continue;
    const int t = vr / G;
    const int g = vr - t * G;
    ushort* op = out + ((int64_t)(s0 + t) * n_q + kh * G + g) * kHD;
#pragma unroll
    for (int nb = 0; nb < kHD / 32; ++nb)
      op[nb * 32 + ln31] = f32_to_bf16(o_acc[nb][r] * inv);
  }
}

}  // namespace

// The caller (paged_attention_prefill, attention_prefill.hip) comes here with
// the shape `s` it validated and attn_plan::hd64_takes' yes. Instantiation
// set of paged_prefill_hd64_kernel: G {1,2,4,7,8} x cache type (10).
void paged_attention_prefill_hd64(torch::Tensor out, torch::Tensor q,
                                  torch::Tensor k_cache, torch::Tensor v_cache,
                                  torch::Tensor block_tables,
                                  torch::Tensor query_start_loc,
                                  torch::Tensor seq_lens, double scale,
                                  const AttnShape& s) {
  const int B = seq_lens.size(0);
  const int64_t Tq = q.size(0);
  TORCH_CHECK(s.hd == kHD && k_cache.size(2) == kBS &&
                  attn_plan::hd64_group(s.G),
              "head_dim 64 prefill: unsupported shape");
  TORCH_CHECK(query_start_loc.numel() == B + 1 && block_tables.size(0) >= B);
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() &&
              v_cache.scalar_type() == k_cache.scalar_type() &&
              k_cache.size(3) == kHD && out.sizes() == q.sizes());
  TORCH_CHECK(attn_plan::hd64_waves(Tq, B, s.n_q, s.n_kv) == kNW,
              "head_dim 64 prefill: bad plan");
  // 16 B loads on q rows and on cache rows (8 B at e5m2)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 &&
                  q.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 16 == 0,
              "head_dim 64 prefill: misaligned q or cache");
  // grid.z covers the longest sequence the batch could hold, Tq tokens
  // (no host copy of query_start_loc); shorter ones exit early
  const int zdim = (int)((Tq * s.G + kROWS - 1) / kROWS);
  dim3 grid(B, s.n_kv, zdim), block(kNW * WAVE_SIZE);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dispatch_int<1, 2, 4, 7, 8>(s.G, "GQA group size", [&](auto g) {
    dispatch_bool(s.fp8_cache, [&](auto fp8) {
      using CT =
          std::conditional_t<decltype(fp8)::value, unsigned char, ushort>;
      hipLaunchKernelGGL(
          (paged_prefill_hd64_kernel<decltype(g)::value, CT>), grid, block, 0,
          stream, (ushort*)out.data_ptr(), (const ushort*)q.data_ptr(),
          (const CT*)k_cache.data_ptr(), (const CT*)v_cache.data_ptr(),
          block_tables.data_ptr<int32_t>(),
          query_start_loc.data_ptr<int32_t>(), seq_lens.data_ptr<int32_t>(),
          (float)scale, s.n_kv, s.max_blocks, q.stride(0));
    });
  });
  HIP_CHECK_KERNEL();
}
