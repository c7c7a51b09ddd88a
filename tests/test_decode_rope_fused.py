"""CPU path of ops.rope_cache_attention_decode: the composition of the refs
(rope, reshape_and_cache, paged_attention_decode, quant_fp8). Caches are
updated in place, q / k / v are left untouched. The GPU kernel is compared
with the two-launch sequence in test_decode_rope_fused_gpu.py.
"""
import math

import pytest
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref

BS = 16


def _case(nq, nkv, hd, lens, cache_dtype, pad_row=None):
    torch.manual_seed(11)
    B = len(lens)
    n_blk = [(L + BS - 1) // BS for L in lens]
    nb = 1 + sum(n_blk)
    bt = torch.zeros(B, max(n_blk), dtype=torch.int32)
    nxt, slots = 1, []
    for b, L in enumerate(lens):
        if b == pad_row:
            slots.append(-1)
            continue
        bt[b, : n_blk[b]] = torch.arange(nxt, nxt + n_blk[b], dtype=torch.int32)
        slots.append(int(bt[b, (L - 1) // BS]) * BS + (L - 1) % BS)
        nxt += n_blk[b]
    return dict(
        q=torch.randn(B, nq, hd, dtype=torch.bfloat16),
        k=torch.randn(B, nkv, hd, dtype=torch.bfloat16),
        v=torch.randn(B, nkv, hd, dtype=torch.bfloat16),
        pos=torch.tensor([L - 1 for L in lens], dtype=torch.int32),
        cs=ref.make_cos_sin_cache(hd, 512, 10000.0),
        kc=torch.randn(nb, nkv, BS, hd).to(cache_dtype),
        vc=torch.randn(nb, nkv, BS, hd).to(cache_dtype),
        slots=torch.tensor(slots, dtype=torch.int64),
        bt=bt,
        seq_lens=torch.tensor(lens, dtype=torch.int32),
        scale=1.0 / math.sqrt(hd),
    )


def _raw(t):
    return t.view(torch.uint8) if t.dtype != torch.bfloat16 else t.view(torch.int16)


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
@pytest.mark.parametrize("fp8_out", [False, True])
@pytest.mark.parametrize(
    "nq,nkv,hd,lens,window,pad_row",
    [
        (8, 2, 64, [1, 16, 17, 33], 0, None),
        (4, 4, 32, [40, 1, 20], 24, 1),
    ],
)
def test_cpu_path_is_the_ref_composition(
    nq, nkv, hd, lens, window, pad_row, fp8_out, cache_dtype
):
    if pad_row is not None:
        lens = [1 if b == pad_row else L for b, L in enumerate(lens)]
    c = _case(nq, nkv, hd, lens, cache_dtype, pad_row)

    # by hand
    kc_a, vc_a = c["kc"].clone(), c["vc"].clone()
    q_r, k_r = ref.rope(c["q"], c["k"], c["pos"], c["cs"])
    ref.reshape_and_cache(k_r, c["v"], kc_a, vc_a, c["slots"])
    out_a = ref.paged_attention_decode(
        q_r, kc_a, vc_a, c["bt"], c["seq_lens"], c["scale"], window=window
    )

    q, k, v = c["q"].clone(), c["k"].clone(), c["v"].clone()
    kc_b, vc_b = c["kc"].clone(), c["vc"].clone()
    out_buf = torch.empty_like(q)
    res = ops.rope_cache_attention_decode(
        q, k, v, c["pos"], c["cs"], kc_b, vc_b, c["slots"], c["bt"],
        c["seq_lens"], c["scale"], out=out_buf, window=window, fp8_out=fp8_out,
    )
    if fp8_out:
        out_b, f8, sc = res
        f8_a, sc_a = ref.quant_fp8(out_a.reshape(len(lens), -1))
        assert torch.equal(f8.view(torch.uint8), f8_a.view(torch.uint8))
        assert torch.equal(sc, sc_a)
    else:
        out_b = res
    assert out_b is out_buf
    assert torch.equal(out_b, out_a)
    assert torch.equal(_raw(kc_b), _raw(kc_a)) and torch.equal(_raw(vc_b), _raw(vc_a))
    assert not torch.equal(_raw(kc_b), _raw(c["kc"]))
    assert not torch.equal(_raw(vc_b), _raw(c["vc"]))
    assert torch.equal(q, c["q"]) and torch.equal(k, c["k"]) and torch.equal(v, c["v"])
    # block 0 (pad rows' block) is never written
    assert torch.equal(_raw(kc_b[0]), _raw(c["kc"][0]))


def test_switch_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("KUBEAI_DECODE_ROPE_FUSED", raising=False)
    assert ops.decode_rope_fused()
    monkeypatch.setenv("KUBEAI_DECODE_ROPE_FUSED", "0")
    assert not ops.decode_rope_fused()
    monkeypatch.setenv("KUBEAI_DECODE_ROPE_FUSED", "1")
    assert ops.decode_rope_fused()
