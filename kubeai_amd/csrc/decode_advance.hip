// decode_advance: the first node of a self-feeding decode graph.
//
// A pure-decode step over an unchanged set of requests has inputs that are a
// function of the step before: the token just sampled, at the next position,
// cached in the slot that the row's block table gives for that position. This
// kernel makes them on the device, in place, from what the replay before left
// behind, so that the graph can be replayed again without the host having
// seen the tokens (runner.py, ModelRunner._run_ahead). A step whose inputs
// were uploaded has b_live[0] == 0 and runs as uploaded. For each row
// b < b_live[0], with p = positions[b] + 1 and i = p / block_size:
//   input_ids[b] = tokens[b];  positions[b] = p;  seq_lens[b] += 1
//   slots[b] = block_tables[b][i] * block_size + p % block_size
// A row with i >= min(n_blocks[b], bt_max) has no block for p yet: it is left
// as it is, reads nothing past its table's filled entries, and a replay
// computes its step again. Pad rows (b >= b_live[0]) are left as they are.
// One thread per row, one small grid, plain stores, integers only.
// Spec: ops/ref.py decode_advance.
#include <torch/extension.h>

#include "common.h"

// v_pk_*_f32 stay out of this file's kernels
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)

namespace {

constexpr int kAdvanceBlock = 64;

__launch_bounds__(kAdvanceBlock) __global__ void decode_advance_kernel(
    int32_t* __restrict__ input_ids,           // [b_pad]
    int32_t* __restrict__ positions,           // [b_pad]
    int64_t* __restrict__ slots,               // [b_pad]
    int32_t* __restrict__ seq_lens,            // [b_pad]
    const int32_t* __restrict__ block_tables,  // [b_pad, bt_max]
    const int32_t* __restrict__ n_blocks,      // [b_pad]
    const int32_t* __restrict__ b_live,        // [1]
    const int64_t* __restrict__ tokens,        // [>= b_pad]
    const int b_pad, const int bt_max, const int block_size) {
  const int b = blockIdx.x * kAdvanceBlock + threadIdx.x;
  if (b >= b_pad || b >= b_live[0]) return;
  const int p = positions[b] + 1;
  const int i = p / block_size;
  if (p < 0 || i >= min(n_blocks[b], bt_max)) return;
  const int64_t block = block_tables[(int64_t)b * bt_max + i];
  input_ids[b] = (int32_t)tokens[b];
  positions[b] = p;
  seq_lens[b] += 1;
  slots[b] = block * block_size + p % block_size;
}

}  // namespace

#pragma clang attribute pop

void decode_advance(torch::Tensor input_ids, torch::Tensor positions,
                    torch::Tensor slots, torch::Tensor seq_lens,
                    torch::Tensor block_tables, torch::Tensor n_blocks,
                    torch::Tensor b_live, torch::Tensor tokens,
                    int64_t block_size) {
  const int64_t b_pad = input_ids.numel();
  auto i32 = [&](const torch::Tensor& t, int64_t n) {
    TORCH_CHECK(t.is_cuda() && t.device() == input_ids.device() &&
                    t.scalar_type() == torch::kInt32 && t.is_contiguous() &&
                    t.numel() == n,
                "decode_advance: int32 tensor of ", n, " elements expected");
  };
  auto i64 = [&](const torch::Tensor& t) {
    TORCH_CHECK(t.is_cuda() && t.device() == input_ids.device() &&
                    t.scalar_type() == torch::kInt64 && t.is_contiguous() &&
                    t.numel() >= b_pad,
                "decode_advance: int64 tensor of at least ", b_pad,
                " elements expected");
  };
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == b_pad);
  TORCH_CHECK(block_size > 0 && block_size <= (1 << 20));
  const int64_t bt_max = block_tables.size(1);
  i32(input_ids, b_pad);
  i32(positions, b_pad);
  i32(seq_lens, b_pad);
  i32(block_tables, b_pad * bt_max);
  i32(n_blocks, b_pad);
  i32(b_live, 1);
  i64(slots);
  i64(tokens);
  TORCH_CHECK(slots.numel() == b_pad);
  if (b_pad == 0) return;
  hipLaunchKernelGGL(
      decode_advance_kernel,
      dim3((unsigned)((b_pad + kAdvanceBlock - 1) / kAdvanceBlock)),
      dim3(kAdvanceBlock), 0, c10::hip::getCurrentHIPStream().stream(),
      input_ids.data_ptr<int32_t>(), positions.data_ptr<int32_t>(),
      slots.data_ptr<int64_t>(), seq_lens.data_ptr<int32_t>(),
      block_tables.data_ptr<int32_t>(), n_blocks.data_ptr<int32_t>(),
      b_live.data_ptr<int32_t>(), tokens.data_ptr<int64_t>(), (int)b_pad,
      (int)bt_max, (int)block_size);
  HIP_CHECK_KERNEL();
}
