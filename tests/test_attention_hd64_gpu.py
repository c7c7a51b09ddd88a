"""head_dim 64 (Llama-3.2-1B, Qwen2 / Qwen2.5-0.5B) on the GPU: the hd-64
prefill and decode kernels against the fp64 oracle of ``attention_oracle``
under its derived bound

    |kernel - out| <= 2**-7 * A + 2**-8 * |out| + 1e-6

(the derivation does not depend on hd), the fp8 output of the decode merge,
the cache write at 128-byte rows, the scope errors, and ``qwen2-tiny-hd64``
through the engine.
"""
import pytest
import torch

import kubeai_amd.ops as ops
from attention_oracle import (
    assert_within_bound,
    make_case,
    oracle_decode,
    oracle_prefill,
)
from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 64
BF16, E5M2 = torch.bfloat16, torch.float8_e5m2
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(E5M2, id="e5m2")]

# the shapes of test_attention_packed_gpu: chunk and wave boundaries inside a
# token's heads, an all-diagonal first chunk (ctx 0), contexts ending inside
# a tile (150) and inside a block (37), a G-row wave (q_len 1)
Q_LENS, CTX, N_KV = [70, 33, 1], [0, 150, 37], 2


def _args(c):
    return (c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["query_start_loc"], c["seq_lens"], c["scale"])


def _dec_args(c):
    return (c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["seq_lens"], c["scale"])


def _check_prefill(c, label):
    q, kc, bt = c["q"], c["k_cache"], c["block_tables"]
    assert ops._C.hd64_prefill_plan(
        q.shape[0], c["seq_lens"].shape[0], q.shape[1], kc.shape[1],
        q.shape[2], bt.shape[1], 0, 0.0)[0] is True
    out, a = oracle_prefill(*_args(c))
    assert_within_bound(ops.paged_attention_prefill(*_args(c)), out, a, label)


def _check_decode(c, n_kv, splits, label):
    B = c["q"].shape[0]
    assert ops._C.decode_plan(B, n_kv, c["block_tables"].shape[1]) == splits
    out, a = oracle_decode(*_dec_args(c))
    assert_within_bound(ops.paged_attention_decode(*_dec_args(c)), out, a,
                        label)


@pytest.mark.parametrize("family", ["randn", "ramp_up"])
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 4, 7, 8])
def test_prefill_hd64(G, cache_dtype, family):
    c = make_case(family, Q_LENS, CTX, N_KV * G, N_KV, hd=HD,
                  cache_dtype=cache_dtype, device=DEV, seed=51)
    _check_prefill(c, f"prefill_hd64/G{G}/{family}")


def test_prefill_hd64_many_chunks():
    """The lengths of test_prefill_packed_many_chunks: 32 ragged sequences,
    one of 116 tokens (812 rows, 4 chunks, the last with 44 rows)."""
    q_lens = [19 + (5 * i) % 13 for i in range(32)]
    q_lens[0] = 116
    ctx = [(37 * i) % 90 for i in range(32)]
    c = make_case("ramp_up", q_lens, ctx, 14, 2, hd=HD, device=DEV, seed=52)
    _check_prefill(c, "prefill_hd64/G7/ragged32/ramp_up")


def test_prefill_hd64_strided_q():
    """q as a view into the fused qkv buffer gives the contiguous call's bits."""
    n_q = 14
    c = make_case("randn", Q_LENS, CTX, n_q, N_KV, hd=HD, cache_dtype=E5M2,
                  device=DEV, seed=53)
    T = c["q"].shape[0]
    qkv = torch.randn(T, (n_q + 2 * N_KV) * HD, dtype=BF16, device=DEV)
    q_view = qkv[:, : n_q * HD].unflatten(-1, (n_q, HD))
    q_view.copy_(c["q"])
    assert not q_view.is_contiguous() and q_view.stride(0) != n_q * HD
    want = ops.paged_attention_prefill(*_args(c))
    got = ops.paged_attention_prefill(*_args(dict(c, q=q_view)))
    assert torch.equal(got, want)


# 16 splits. 19, 33: splits of one block (a half-empty pair); 257: 17 blocks
# in chunks of 2, the last split unpaired; 700: 44 blocks in chunks of 3, the
# second pair of a split straddles blk_hi; 1, 16: one row, one full block
_DEC_LENS = [257, 64, 19, 100, 1, 16, 17, 33, 700]


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 2, 4, 7, 8])
def test_decode_hd64(G, cache_dtype):
    B = len(_DEC_LENS)
    c = make_case("randn", [1] * B, [L - 1 for L in _DEC_LENS], N_KV * G,
                  N_KV, hd=HD, cache_dtype=cache_dtype, device=DEV, seed=54)
    _check_decode(c, N_KV, 16, f"decode_hd64/G{G}/randn")


@pytest.mark.parametrize("cache_dtype", DTYPES)
def test_decode_hd64_needle_sweep(cache_dtype):
    """90 rows of L = 720 (45 blocks, chunks of 3 at 16 splits), the needle
    at 8 * i + i % 8: every block and both halves of every pair are hit, and
    a token lost at a block, half-wave, wave or split boundary is O(1)."""
    B = 90
    c = make_case("needle", [1] * B, [719] * B, 4, 1, hd=HD,
                  cache_dtype=cache_dtype, device=DEV, seed=55,
                  needle_pos=[8 * i + i % 8 for i in range(B)])
    _check_decode(c, 1, 16, "decode_hd64/G4/needle")


def _no_split_case():
    B = 256
    return make_case("randn", [1] * B, [(37 * i) % 90 for i in range(B)], 32,
                     8, hd=HD, device=DEV, seed=56)


def test_decode_hd64_no_split():
    """B * n_kv = 2048 workgroups: one split, the kernel writes bf16 itself."""
    _check_decode(_no_split_case(), 8, 1, "decode_hd64/G4/no_split")


@pytest.mark.parametrize("split", [16, 1])
def test_decode_hd64_fp8_out(split):
    if split == 1:
        c, n_kv = _no_split_case(), 8
    else:
        B, n_kv = len(_DEC_LENS), N_KV
        c = make_case("randn", [1] * B, [L - 1 for L in _DEC_LENS], 14, n_kv,
                      hd=HD, cache_dtype=E5M2, device=DEV, seed=57)
    B = c["q"].shape[0]
    assert ops._C.decode_plan(B, n_kv, c["block_tables"].shape[1]) == split
    out = ops.paged_attention_decode(*_dec_args(c))
    want8, want_scale = ops.quant_fp8(out.view(B, -1))
    got, got8, got_scale = ops.paged_attention_decode(*_dec_args(c),
                                                      fp8_out=True)
    assert torch.equal(got, out)
    assert torch.equal(got8.view(torch.uint8), want8.view(torch.uint8))
    assert torch.equal(got_scale, want_scale)


@pytest.mark.parametrize("cache_dtype", DTYPES)
def test_rope_and_cache_hd64(cache_dtype):
    """128-byte rows: q, k and both caches bit-equal to the reference."""
    torch.manual_seed(58)
    T, nq, nkv, nb = 5, 14, 2, 4
    q = torch.randn(T, nq, HD, dtype=BF16, device=DEV)
    k = torch.randn(T, nkv, HD, dtype=BF16, device=DEV)
    v = torch.randn(T, nkv, HD, dtype=BF16, device=DEV)
    pos = torch.randint(0, 4000, (T,), dtype=torch.int32, device=DEV)
    cs = ref.make_cos_sin_cache(HD, 4096, 500000.0).to(DEV)
    slots = torch.tensor([17, 3, -1, 63, 0], dtype=torch.int64, device=DEV)
    kc = torch.randn(nb, nkv, 16, HD, device=DEV).to(cache_dtype)
    vc = torch.randn(nb, nkv, 16, HD, device=DEV).to(cache_dtype)
    kc_ref, vc_ref = kc.cpu(), vc.cpu()
    q_ref, k_ref = ref.rope(q.cpu(), k.cpu(), pos.cpu(), cs.cpu())
    ref.reshape_and_cache(k_ref, v.cpu(), kc_ref, vc_ref, slots.cpu())
    ops.rope_and_cache(q, k, v, pos, cs, kc, vc, slots)
    assert torch.equal(q.cpu(), q_ref) and torch.equal(k.cpu(), k_ref)
    assert torch.equal(kc.cpu().view(torch.uint8), kc_ref.view(torch.uint8))
    assert torch.equal(vc.cpu().view(torch.uint8), vc_ref.view(torch.uint8))


def test_hd64_scope():
    plan = ops._C.hd64_prefill_plan
    assert plan(104, 3, 14, 2, 64, 12) == (True, 8)
    assert plan(104, 3, 14, 2, 128, 12)[0] is False           # hd 128
    assert plan(104, 3, 14, 2, 64, 12, 48, 0.0)[0] is False   # window
    assert plan(104, 3, 14, 2, 64, 12, 0, 50.0)[0] is False   # softcap
    assert plan(104, 3, 6, 2, 64, 12)[0] is False             # G = 3
    c = make_case("randn", [40], [20], 14, 2, hd=HD, device=DEV, seed=59)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.paged_attention_prefill(*_args(c), window=48)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.paged_attention_append(*_args(c))
    d = make_case("randn", [1], [59], 14, 2, hd=HD, device=DEV, seed=59)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        ops.paged_attention_decode(*_dec_args(d), window=48)


def _generate(seed=11, **kw):
    eng = LLMEngine(EngineConfig(
        model="qwen2-tiny-hd64", device=DEV, max_model_len=512,
        num_gpu_blocks=256, seed=seed, **kw))
    eng.add_request(list(range(10, 100)),
                    SamplingParams(max_tokens=8, ignore_eos=True),
                    request_id="x")
    for _ in range(100):
        for o in eng.step():
            if o.finished:
                return o.output_token_ids
    raise AssertionError("did not finish")


def test_qwen2_hd64_engine_gpu():
    """Prefill, then pure-decode steps through rope_cache_attention_decode's
    two-launch branch and the decode graph."""
    a, b = _generate(), _generate()
    assert len(a) == 8 and a == b
    # chunked prefill: 32-token chunks over a growing cached context
    assert len(_generate(max_num_batched_tokens=32)) == 8
    assert len(_generate(quantization="fp8")) == 8
