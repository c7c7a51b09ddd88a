"""ops.paged_attention_append off the GPU is the reference prefill."""
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref
from attention_oracle import make_case


def test_append_cpu_is_ref():
    c = make_case("randn", [5, 17], [40, 0], 4, 2)
    args = (c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["query_start_loc"], c["seq_lens"], c["scale"])
    assert torch.equal(ops.paged_attention_append(*args, n_splits=3),
                       ref.paged_attention_prefill(*args))
