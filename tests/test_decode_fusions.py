"""CPU fallbacks of the fused decode-layer ops equal their reference
sequences (ref.rope + ref.reshape_and_cache; reference decode attention +
ref.quant_fp8)."""
import math

import pytest
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(99)


@pytest.mark.parametrize("layout", ["qkv_views", "separate"])
def test_rope_and_cache_cpu_equals_reference_sequence(layout):
    T, nq, nkv, hd, nb, bs = 5, 4, 2, 16, 3, 4
    qkv = torch.randn(T, (nq + 2 * nkv) * hd, dtype=torch.bfloat16)
    q, k, v = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    q = q.unflatten(-1, (nq, hd))
    k = k.unflatten(-1, (nkv, hd))
    v = v.unflatten(-1, (nkv, hd))
    if layout == "separate":
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    pos = torch.randint(0, 60, (T,), dtype=torch.int32)
    cs = ref.make_cos_sin_cache(hd, 64, 10000.0)
    slots = torch.randperm(nb * bs)[:T].to(torch.int64)
    slots[1] = -1
    kc0 = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16)
    vc0 = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16)

    q_a, k_a = ref.rope(q, k, pos, cs)
    kc_a, vc_a = kc0.clone(), vc0.clone()
    ref.reshape_and_cache(k_a, v, kc_a, vc_a, slots)

    kc_b, vc_b = kc0.clone(), vc0.clone()
    q_b, k_b = ops.rope_and_cache(q, k, v, pos, cs, kc_b, vc_b, slots)

    assert torch.equal(q_b, q_a) and torch.equal(k_b, k_a)
    assert torch.equal(kc_b, kc_a) and torch.equal(vc_b, vc_a)
    assert not torch.equal(kc_b, kc0)
    # only the T-1 valid slots were written (the pad row wrote nothing)
    changed = (kc_b != kc0).any(-1).any(1)  # [nb, bs]
    assert int(changed.sum()) == T - 1


@pytest.mark.parametrize("with_out", [False, True])
def test_decode_fp8_out_cpu_equals_reference_sequence(with_out):
    nq, nkv, hd, bs = 4, 2, 16, 16
    lens = [30, 7, 1]
    B = len(lens)
    max_blocks = max((L + bs - 1) // bs for L in lens)
    nb = B * max_blocks + 1
    kc = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16)
    vc = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16)
    bt = torch.arange(1, nb, dtype=torch.int32).reshape(B, max_blocks)
    seq_lens = torch.tensor(lens, dtype=torch.int32)
    q = torch.randn(B, nq, hd, dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(hd)

    want = ref.paged_attention_decode(q, kc, vc, bt, seq_lens, scale)
    want8, want_scale = ref.quant_fp8(want.reshape(B, -1))

    buf = torch.empty_like(q) if with_out else None
    out, o8, oscale = ops.paged_attention_decode(
        q, kc, vc, bt, seq_lens, scale, out=buf, fp8_out=True
    )
    if with_out:
        assert out is buf
    assert torch.equal(out, want)
    assert torch.equal(o8.view(torch.uint8), want8.view(torch.uint8))
    assert torch.equal(oscale, want_scale)
    # without fp8_out the return stays a single tensor
    plain = ops.paged_attention_decode(q, kc, vc, bt, seq_lens, scale)
    assert torch.equal(plain, want)
