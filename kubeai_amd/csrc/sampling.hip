// Token sampling kernels (two-stage argmax reduction).
//
// greedy_sample:  argmax over the vocab row.
// gumbel_sample:  argmax(logits/T + Gumbel noise) — exact temperature
//   sampling without softmax or sort. RNG = counter-based splitmix64 hash
//   (common.h), spec-identical to ops/ref.py.
// Tie-break: lowest index wins (matches torch.argmax).
// *_sample_logprob: the same token, plus its log-probability and the row's
//   logsumexp, from the same two launches.
// token_logprobs: log-probability of given tokens, one launch.
//
// Stage 1 splits each vocab row into kSplits chunks (B*kSplits workgroups
// keep all 256 CUs busy even at decode batch ~32); stage 2 is one wave per
// row reducing the partials.
//
// logsumexp. Every split i yields (m_i, s_i) over the RAW logits of its
// chunk (not the Gumbel-perturbed values): m_i the chunk maximum, s_i =
// sum of expf(x - m_i). Per thread the terms are added in increasing v,
// then the 64 lanes by xor butterfly, then the 4 waves in increasing order.
// An empty or all -inf chunk gives (-inf, 0). One wave merges a row:
//   M = max m_i;  S = sum of s_i * expf(m_i - M) in increasing i
//   lse = logf(S) + M;  logprob = logits[token] - lse
// No atomics and one fixed order, so results are bit-identical from run to
// run, and between the two-stage sampler and token_logprobs, which walks the
// same chunks with the same thread mapping inside one workgroup.
//
// Logits are fp32 or bf16 (the lm_head GEMM's own output type). A bf16 logit
// widens to fp32 exactly, and all arithmetic is on the widened value, so
// token, logprob and lse are bit-identical to a run on logits.float(). Loads
// are one element per lane: no row alignment is assumed (a bf16 row of odd V
// starts 2 B aligned).
#include <torch/extension.h>

#include <type_traits>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / WAVE_SIZE;
constexpr int kSplits = 32;
// a chunk of up to kBlock * kRegIters logits (V <= 131072) stays in
// registers between the max sweep and the expf sweep; a longer one is read
// again (from L2)
constexpr int kRegIters = 16;

// LT = logits element: float, or ushort holding bf16 bits
DEV_INLINE float logit_f32(const float x) { return x; }
DEV_INLINE float logit_f32(const ushort x) { return bf16_to_f32(x); }

DEV_INLINE float max_waves(const float (&s)[kWaves]) {
  return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

// the pinned order of the last step of a chunk's sum
DEV_INLINE float sum_waves(const float (&s)[kWaves]) {
  return ((s[0] + s[1]) + s[2]) + s[3];
}
static_assert(kWaves == 4, "max_waves / sum_waves spell four waves");

// expf(x - m) with m the chunk maximum; an all -inf chunk sums to 0, not NaN
DEV_INLINE float exp_ref(const float m) { return m == -INFINITY ? 0.f : m; }

// One wave; lane i < kSplits holds (m_i, s_i), the other lanes (-inf, 0).
// Every lane returns the row's logsumexp.
DEV_INLINE float merge_lse(const float m, const float s) {
  const float M = wave_reduce_max(m);
  const float t = (m == -INFINITY) ? 0.f : s * expf(m - M);
  float S = 0.f;
#pragma unroll
  for (int i = 0; i < kSplits; ++i) S += __shfl(t, i, 64);
  return logf(S) + M;
}

struct SamplePartials {  // each [B, kSplits]
  float* val;            // best (perturbed) value of the split
  int32_t* idx;          // its vocab index
  float* m;              // kLse: max of the raw logits
  float* s;              // kLse: sum of expf(x - m)
};

template <typename LT, bool kGumbel, bool kLse, bool kRegs>
__launch_bounds__(kBlock) __global__ void sample_stage1(
    const SamplePartials part,
    const LT* __restrict__ logits,          // [B, V]
    const float* __restrict__ temperature,  // [B]
    const int64_t* __restrict__ seeds,      // [B]
    const int64_t step, const int V) {
  static_assert(kLse || !kRegs, "registers serve the second sweep only");
  const int b = blockIdx.x;
  const int split = blockIdx.y;
  const int chunk = (V + kSplits - 1) / kSplits;
  const int lo = split * chunk;
  const int hi = min(V, lo + chunk);
  const LT* row = logits + (int64_t)b * V;
  float temp = 1.0f;
  uint64_t key = 0;
  bool greedy = !kGumbel;
  if constexpr (kGumbel) {
    temp = temperature[b];
    if (temp <= 0.f) greedy = true;
    key = (uint64_t)seeds[b] * 1000003ull + (uint64_t)step;
  }

  float best = -INFINITY;
  int best_idx = V;
  float m = -INFINITY;
  auto visit = [&](const int v, const float raw) {
    float val = raw;
    if (!greedy) {
      float u = hash_uniform(key, (uint64_t)v);
      val = val / temp + (-__logf(-__logf(u)));
    }
    if (val > best || (val == best && v < best_idx)) {
      best = val;
      best_idx = v;
    }
    if constexpr (kLse) m = fmaxf(m, raw);
  };
  float x[kRegs ? kRegIters : 1];
  if constexpr (kRegs) {
    // all loads first, then the sweep: x[] is indexed by constants only
    if constexpr (std::is_same_v<LT, float>) {
#pragma unroll
      for (int it = 0; it < kRegIters; ++it) {
        const int v = lo + threadIdx.x + it * kBlock;
        x[it] = v < hi ? row[v] : -INFINITY;
      }
    } else {
      // bf16: behind the `v < hi` guard the compiler widened each element
      // next to its load and waited on the 16 loads one by one (13.5 us
      // against 8.8 us for fp32 at 40 x 128256,
      // profiles/r09_decode_step.md). Unguarded loads at an index clamped
      // into the row go out together; the guard moves to the widening.
      uint32_t raw[kRegIters];
#pragma unroll
      for (int it = 0; it < kRegIters; ++it)
        raw[it] = row[min(lo + (int)threadIdx.x + it * kBlock, V - 1)];
#pragma unroll
      for (int it = 0; it < kRegIters; ++it) {
        const int v = lo + threadIdx.x + it * kBlock;
        x[it] = v < hi ? logit_f32((ushort)raw[it]) : -INFINITY;
      }
    }
#pragma unroll
    for (int it = 0; it < kRegIters; ++it) {
      const int v = lo + threadIdx.x + it * kBlock;
      if (v < hi) visit(v, x[it]);
    }
  } else {
    for (int v = lo + threadIdx.x; v < hi; v += kBlock)
      visit(v, logit_f32(row[v]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, 64);
    int oi = __shfl_xor(best_idx, off, 64);
    if (ov > best || (ov == best && oi < best_idx)) {
      best = ov;
      best_idx = oi;
    }
  }
  if constexpr (kLse) m = wave_reduce_max(m);
  __shared__ float sval[kWaves];
  __shared__ int sidx[kWaves];
  __shared__ float smax[kWaves];
  __shared__ float ssum[kWaves];
  const int wave = threadIdx.x / WAVE_SIZE;
  if (threadIdx.x % WAVE_SIZE == 0) {
    sval[wave] = best;
    sidx[wave] = best_idx;
    if constexpr (kLse) smax[wave] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      if (sval[w] > best || (sval[w] == best && sidx[w] < best_idx)) {
        best = sval[w];
        best_idx = sidx[w];
      }
    }
    part.val[b * kSplits + split] = best;
    part.idx[b * kSplits + split] = best_idx;
  }
  if constexpr (kLse) {
    m = max_waves(smax);
    const float ref = exp_ref(m);
    float s = 0.f;
    if constexpr (kRegs) {
#pragma unroll
      for (int it = 0; it < kRegIters; ++it) {
        const int v = lo + threadIdx.x + it * kBlock;
        if (v < hi) s += expf(x[it] - ref);
      }
    } else {
      for (int v = lo + threadIdx.x; v < hi; v += kBlock)
        s += expf(logit_f32(row[v]) - ref);
    }
    s = wave_reduce_sum(s);
    if (threadIdx.x % WAVE_SIZE == 0) ssum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      part.m[b * kSplits + split] = m;
      part.s[b * kSplits + split] = sum_waves(ssum);
    }
  }
}

template <typename LT, bool kLse>
__global__ void sample_stage2(int64_t* __restrict__ out,
                              float* __restrict__ out_logprob,  // kLse
                              float* __restrict__ out_lse,      // kLse
                              const SamplePartials part,
                              const LT* __restrict__ logits,  // kLse
                              const int V) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  float best = (lane < kSplits) ? part.val[b * kSplits + lane] : -INFINITY;
  int best_idx = (lane < kSplits) ? part.idx[b * kSplits + lane] : INT32_MAX;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, 64);
    int oi = __shfl_xor(best_idx, off, 64);
    if (ov > best || (ov == best && oi < best_idx)) {
      best = ov;
      best_idx = oi;
    }
  }
  if constexpr (kLse) {
    const float lse =
        merge_lse((lane < kSplits) ? part.m[b * kSplits + lane] : -INFINITY,
                  (lane < kSplits) ? part.s[b * kSplits + lane] : 0.f);
    if (lane == 0) {
      // a row of NaNs has no argmax (index V, as greedy_sample reports it)
      const float xt =
          best_idx < V ? logit_f32(logits[(int64_t)b * V + best_idx]) : (float)NAN;
      out_logprob[b] = xt - lse;
      out_lse[b] = lse;
    }
  }
  if (lane == 0) out[b] = best_idx;
}

// logprob of tokens[b] and the row's logsumexp in one launch: group g of
// kBlock threads takes splits g, g + kGroups, ... and computes each one's
// (m, s) as sample_stage1 does; wave 0 then merges them as sample_stage2 does.
constexpr int kGroups = 4;
static_assert(kSplits % kGroups == 0, "every group runs every round");

template <typename LT>
__launch_bounds__(kBlock* kGroups) __global__ void token_logprobs_kernel(
    float* __restrict__ out_logprob,    // [B]
    float* __restrict__ out_lse,        // [B]
    const LT* __restrict__ logits,      // [B, V]
    const int64_t* __restrict__ tokens,  // [B]
    const int V) {
  const int b = blockIdx.x;
  const int g = threadIdx.x / kBlock;
  const int tid = threadIdx.x % kBlock;
  const int wave = tid / WAVE_SIZE;
  const LT* row = logits + (int64_t)b * V;
  const int chunk = (V + kSplits - 1) / kSplits;
  __shared__ float smax[kGroups][kWaves];
  __shared__ float ssum[kGroups][kWaves];
  __shared__ float pm[kSplits];
  __shared__ float ps[kSplits];
  for (int r = 0; r < kSplits / kGroups; ++r) {
    const int split = r * kGroups + g;
    const int lo = split * chunk;
    const int hi = min(V, lo + chunk);
    float m = -INFINITY;
    for (int v = lo + tid; v < hi; v += kBlock)
      m = fmaxf(m, logit_f32(row[v]));
    m = wave_reduce_max(m);
    if (tid % WAVE_SIZE == 0) smax[g][wave] = m;
    __syncthreads();
    m = max_waves(smax[g]);
    const float ref = exp_ref(m);
    float s = 0.f;
    for (int v = lo + tid; v < hi; v += kBlock)
      s += expf(logit_f32(row[v]) - ref);
    s = wave_reduce_sum(s);
    if (tid % WAVE_SIZE == 0) ssum[g][wave] = s;
    __syncthreads();
    if (tid == 0) {
      pm[split] = m;
      ps[split] = sum_waves(ssum[g]);
    }
  }
  __syncthreads();
  if (threadIdx.x < WAVE_SIZE) {
    const int lane = threadIdx.x;
    const float lse = merge_lse((lane < kSplits) ? pm[lane] : -INFINITY,
                                (lane < kSplits) ? ps[lane] : 0.f);
    if (lane == 0) {
      const int64_t t = tokens[b];
      const float xt = (t >= 0 && t < V) ? logit_f32(row[t]) : (float)NAN;
      out_logprob[b] = xt - lse;
      out_lse[b] = lse;
    }
  }
}

void check_logits(const torch::Tensor& logits) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32 ||
                  logits.scalar_type() == torch::kBFloat16,
              "sampling expects fp32 or bf16 logits");
}

// calls f with a null pointer of the kernels' element type for `logits`
template <typename F>
void dispatch_logits(const torch::Tensor& logits, F&& f) {
  if (logits.scalar_type() == torch::kBFloat16)
    f(static_cast<const ushort*>(nullptr));
  else
    f(static_cast<const float*>(nullptr));
}

// [B] outputs of the dtype T on the device of `logits`
template <typename T>
T* row_output(const torch::Tensor& t, const torch::Tensor& logits) {
  TORCH_CHECK(t.is_contiguous() && t.numel() == logits.size(0) &&
              t.device() == logits.device());
  return t.data_ptr<T>();
}

template <bool kGumbel, bool kLse>
void launch_sample(int64_t* out, float* out_logprob, float* out_lse,
                   const torch::Tensor& logits, const float* temp_ptr,
                   const int64_t* seed_ptr, int64_t step) {
  const int B = logits.size(0), V = logits.size(1);
  if (B == 0) return;
  // one allocation: val | idx | m | s, each [B, kSplits] 4-byte words
  const int64_t n = (int64_t)B * kSplits;
  auto buf = torch::empty(
      {(kLse ? 4 : 2) * n},
      torch::TensorOptions().device(logits.device()).dtype(torch::kInt32));
  int32_t* w = buf.data_ptr<int32_t>();
  const SamplePartials part{reinterpret_cast<float*>(w), w + n,
                            kLse ? reinterpret_cast<float*>(w + 2 * n) : nullptr,
                            kLse ? reinterpret_cast<float*>(w + 3 * n) : nullptr};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int chunk = (V + kSplits - 1) / kSplits;
  dispatch_logits(logits, [&](auto null_lt) {
    using LT = std::remove_const_t<std::remove_pointer_t<decltype(null_lt)>>;
    const LT* lp = static_cast<const LT*>(logits.data_ptr());
    dispatch_bool(kLse && chunk <= kBlock * kRegIters, [&](auto regs) {
      constexpr bool kRegs = kLse && decltype(regs)::value;
      hipLaunchKernelGGL((sample_stage1<LT, kGumbel, kLse, kRegs>),
                         dim3(B, kSplits), dim3(kBlock), 0, stream, part, lp,
                         temp_ptr, seed_ptr, step, V);
    });
    HIP_CHECK_KERNEL();
    hipLaunchKernelGGL((sample_stage2<LT, kLse>), dim3(B), dim3(WAVE_SIZE), 0,
                       stream, out, out_logprob, out_lse, part, lp, V);
    HIP_CHECK_KERNEL();
  });
}

void check_gumbel(const torch::Tensor& logits, const torch::Tensor& temperature,
                  const torch::Tensor& seeds) {
  TORCH_CHECK(temperature.scalar_type() == torch::kFloat32);
  TORCH_CHECK(seeds.scalar_type() == torch::kInt64);
  TORCH_CHECK(temperature.is_contiguous() && seeds.is_contiguous());
  TORCH_CHECK(temperature.numel() == logits.size(0) &&
              seeds.numel() == logits.size(0));
}

}  // namespace

void greedy_sample(torch::Tensor out, torch::Tensor logits) {
  check_logits(logits);
  launch_sample<false, false>(row_output<int64_t>(out, logits), nullptr,
                              nullptr, logits, nullptr, nullptr, 0);
}

void gumbel_sample(torch::Tensor out, torch::Tensor logits,
                   torch::Tensor temperature, torch::Tensor seeds,
                   int64_t step) {
  check_logits(logits);
  check_gumbel(logits, temperature, seeds);
  launch_sample<true, false>(row_output<int64_t>(out, logits), nullptr, nullptr,
                             logits, temperature.data_ptr<float>(),
                             seeds.data_ptr<int64_t>(), step);
}

void greedy_sample_logprob(torch::Tensor out, torch::Tensor out_logprob,
                           torch::Tensor out_lse, torch::Tensor logits) {
  check_logits(logits);
  launch_sample<false, true>(row_output<int64_t>(out, logits),
                             row_output<float>(out_logprob, logits),
                             row_output<float>(out_lse, logits), logits,
                             nullptr, nullptr, 0);
}

void gumbel_sample_logprob(torch::Tensor out, torch::Tensor out_logprob,
                           torch::Tensor out_lse, torch::Tensor logits,
                           torch::Tensor temperature, torch::Tensor seeds,
                           int64_t step) {
  check_logits(logits);
  check_gumbel(logits, temperature, seeds);
  launch_sample<true, true>(row_output<int64_t>(out, logits),
                            row_output<float>(out_logprob, logits),
                            row_output<float>(out_lse, logits), logits,
                            temperature.data_ptr<float>(),
                            seeds.data_ptr<int64_t>(), step);
}

void token_logprobs(torch::Tensor out_logprob, torch::Tensor out_lse,
                    torch::Tensor logits, torch::Tensor tokens) {
  check_logits(logits);
  TORCH_CHECK(tokens.scalar_type() == torch::kInt64);
  const int B = logits.size(0), V = logits.size(1);
  float* lp = row_output<float>(out_logprob, logits);
  float* lse = row_output<float>(out_lse, logits);
  const int64_t* tok = row_output<int64_t>(tokens, logits);
  if (B == 0) return;
  dispatch_logits(logits, [&](auto null_lt) {
    using LT = std::remove_const_t<std::remove_pointer_t<decltype(null_lt)>>;
    hipLaunchKernelGGL(token_logprobs_kernel<LT>, dim3(B),
                       dim3(kBlock * kGroups), 0,
                       c10::hip::getCurrentHIPStream().stream(), lp, lse,
                       static_cast<const LT*>(logits.data_ptr()), tok, V);
  });
  HIP_CHECK_KERNEL();
}

// ---------------------------------------------------------------------
// Rejection-based nucleus sampling support (runner._sample_topk_topp):
// one pass computes per-row softmax stats; per candidate draw another
// single pass decides membership (probability mass strictly above the
// sampled logit < top_p, and rank < top_k) — no [S,V] intermediates.

namespace {

__global__ void nucleus_stats_kernel(
    float* __restrict__ m_out, float* __restrict__ z_out,
    const float* __restrict__ logits, const float* __restrict__ temps,
    const int V) {
  const int row = blockIdx.x;
  const float* x = logits + (int64_t)row * V;
  const float t = fmaxf(temps[row], 1e-6f);
  __shared__ float red[16];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += blockDim.x) m = fmaxf(m, x[i]);
  m = wave_reduce_max(m);
  const int wave = threadIdx.x / WAVE_SIZE, lane = threadIdx.x % WAVE_SIZE;
  const int nw = blockDim.x / WAVE_SIZE;
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float mm = -INFINITY;
  for (int w = 0; w < nw; ++w) mm = fmaxf(mm, red[w]);
  __syncthreads();
  float z = 0.f;
  for (int i = threadIdx.x; i < V; i += blockDim.x)
    z += __expf((x[i] - mm) / t);
  z = block_reduce_sum(z, red);
  if (threadIdx.x == 0) {
    m_out[row] = mm;
    z_out[row] = z;
  }
}

__global__ void nucleus_accept_kernel(
    unsigned char* __restrict__ ok,      // [S]
    const float* __restrict__ logits,    // [S, V]
    const int64_t* __restrict__ cand,    // [S]
    const float* __restrict__ m_in, const float* __restrict__ z_in,
    const float* __restrict__ temps, const float* __restrict__ top_ps,
    const int32_t* __restrict__ top_ks, const int V) {
  const int row = blockIdx.x;
  const float t0 = temps[row];
  if (t0 <= 0.f) {  // greedy rows: argmax is always in the nucleus
    if (threadIdx.x == 0) ok[row] = 1;
    return;
  }
  const float* x = logits + (int64_t)row * V;
  const float lt = x[cand[row]];
  const float t = fmaxf(t0, 1e-6f);
  const float m = m_in[row], z = z_in[row];
  __shared__ float red[16];
  float mass = 0.f;
  int cnt = 0;
  for (int i = threadIdx.x; i < V; i += blockDim.x) {
    const float xi = x[i];
    if (xi > lt) {
      mass += __expf((xi - m) / t);
      ++cnt;
    }
  }
  mass = block_reduce_sum(mass, red);
  __syncthreads();
  float cntf = block_reduce_sum((float)cnt, red);
  if (threadIdx.x == 0) {
    const float mass_above = mass / z;
    const int k = top_ks[row];
    ok[row] = (mass_above < top_ps[row] && (k <= 0 || (int)cntf < k)) ? 1 : 0;
  }
}

}  // namespace

void nucleus_stats(torch::Tensor m, torch::Tensor z, torch::Tensor logits,
                   torch::Tensor temps) {
  TORCH_CHECK(logits.is_contiguous() &&
              logits.scalar_type() == torch::kFloat32);
  const int S = logits.size(0), V = logits.size(1);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(nucleus_stats_kernel, dim3(S), dim3(512), 0, stream,
                     m.data_ptr<float>(), z.data_ptr<float>(),
                     logits.data_ptr<float>(), temps.data_ptr<float>(), V);
  HIP_CHECK_KERNEL();
}

void nucleus_accept(torch::Tensor ok, torch::Tensor logits,
                    torch::Tensor cand, torch::Tensor m, torch::Tensor z,
                    torch::Tensor temps, torch::Tensor top_ps,
                    torch::Tensor top_ks) {
  TORCH_CHECK(logits.is_contiguous() &&
              logits.scalar_type() == torch::kFloat32);
  TORCH_CHECK(cand.scalar_type() == torch::kInt64);
  TORCH_CHECK(top_ks.scalar_type() == torch::kInt32);
  const int S = logits.size(0), V = logits.size(1);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(nucleus_accept_kernel, dim3(S), dim3(512), 0, stream,
                     ok.data_ptr<unsigned char>(),
                     logits.data_ptr<float>(), cand.data_ptr<int64_t>(),
                     m.data_ptr<float>(), z.data_ptr<float>(),
                     temps.data_ptr<float>(), top_ps.data_ptr<float>(),
                     top_ks.data_ptr<int32_t>(), V);
  HIP_CHECK_KERNEL();
}
