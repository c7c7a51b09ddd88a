"""GQA group sizes 5, 6 and 7 (the Qwen2 family) on the GPU: the packed-row
prefill kernel and the G = 7 decode against the fp64 oracle of
``attention_oracle`` under its derived bound

    |kernel - out| <= 2**-7 * A + 2**-8 * |out| + 1e-6

(the packed kernel rounds P to bf16 and sums l from the unrounded p, the
terms that bound was derived from), and ``qwen2-tiny-g7`` through the engine.
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
from test_decode_rope_fused_gpu import _check as check_fused_equals_two_launches

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, E5M2 = torch.bfloat16, torch.float8_e5m2
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(E5M2, id="e5m2")]

# n_kv = 2: a wrong kv_head * G + g reads the other group's heads. At G = 7 a
# 256-row chunk holds 36 4/7 tokens and a 32-row wave 4 4/7, so chunk and wave
# boundaries fall inside a token's heads (70 tokens are 2 chunks at every G);
# q_len 1 is G rows in one partly filled wave; ctx 150 and 37 end inside a KV
# tile and inside a cache block; ctx 0 with 70 tokens makes the first tiles
# diagonal.
Q_LENS, CTX, N_KV = [70, 33, 1], [0, 150, 37], 2


def _args(c):
    return (c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["query_start_loc"], c["seq_lens"], c["scale"])


def _check_prefill(c, label):
    assert _packed_plan(c) == (True, 8)  # one width: 8 waves, 256 rows
    out, a = oracle_prefill(*_args(c))
    assert_within_bound(ops.paged_attention_prefill(*_args(c)), out, a, label)


def _packed_plan(c, window=0, softcap=0.0):
    q, kc, bt = c["q"], c["k_cache"], c["block_tables"]
    return ops._C.packed_prefill_plan(
        q.shape[0], c["seq_lens"].shape[0], q.shape[1], kc.shape[1],
        q.shape[2], bt.shape[1], window, softcap)


@pytest.mark.parametrize("family", ["randn", "ramp_up"])
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("G", [5, 6, 7])
def test_prefill_packed(G, cache_dtype, family):
    """ramp_up puts the mass on the last allowed key, so a limit taken from r
    instead of r / G, or off by one, misses the bound by 10x or more."""
    c = make_case(family, Q_LENS, CTX, N_KV * G, N_KV,
                  cache_dtype=cache_dtype, device=DEV, seed=41)
    _check_prefill(c, f"prefill_packed/G{G}/{family}")


def test_prefill_packed_many_chunks():
    """32 ragged sequences, one of 116 tokens (812 rows, 4 chunks, the last
    with 44 rows: one full wave, one of 12 rows, six empty)."""
    q_lens = [19 + (5 * i) % 13 for i in range(32)]
    q_lens[0] = 116
    ctx = [(37 * i) % 90 for i in range(32)]
    c = make_case("ramp_up", q_lens, ctx, 14, 2, device=DEV, seed=42)
    _check_prefill(c, "prefill_packed/G7/ragged32/ramp_up")


def test_prefill_packed_strided_q():
    """q as a view into the fused qkv buffer gives the contiguous call's bits."""
    n_q, hd = 14, 128
    c = make_case("randn", Q_LENS, CTX, n_q, N_KV, cache_dtype=E5M2,
                  device=DEV, seed=43)
    T = c["q"].shape[0]
    qkv = torch.randn(T, (n_q + 2 * N_KV) * hd, dtype=BF16, device=DEV)
    q_view = qkv[:, : n_q * hd].unflatten(-1, (n_q, hd))
    q_view.copy_(c["q"])
    assert not q_view.is_contiguous() and q_view.stride(0) != n_q * hd
    want = ops.paged_attention_prefill(*_args(c))
    got = ops.paged_attention_prefill(*_args(dict(c, q=q_view)))
    assert torch.equal(got, want)


def test_packed_plan_scope():
    plan = ops._C.packed_prefill_plan
    for G in (5, 6, 7):
        assert plan(104, 3, 2 * G, 2, 128, 12)[0] is True
    assert plan(104, 3, 6, 2, 128, 12)[0] is False           # G = 3
    assert plan(104, 3, 8, 2, 128, 12)[0] is False           # G = 4
    assert plan(104, 3, 14, 2, 256, 12)[0] is False          # hd 256
    assert plan(104, 3, 14, 2, 128, 12, 48, 0.0)[0] is False  # window
    assert plan(104, 3, 14, 2, 128, 12, 0, 50.0)[0] is False  # softcap
    assert plan(1, 1, 7, 1, 128, 1) == (True, 8)
    assert plan(8192, 4, 28, 4, 128, 512) == (True, 8)
    c = make_case("randn", [40], [20], 14, 2, device=DEV, seed=44)
    with pytest.raises(RuntimeError, match="unsupported GQA group size"):
        ops.paged_attention_prefill(*_args(c), window=48)


# the lengths of test_attention_paths_gpu.test_decode_other_group_sizes
_DEC_LENS = [257, 64, 19, 100, 1, 16, 17]


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("hd", [128, 256])
def test_decode_g7(hd, cache_dtype):
    B = len(_DEC_LENS)
    c = make_case("randn", [1] * B, [L - 1 for L in _DEC_LENS], 14, 2, hd=hd,
                  cache_dtype=cache_dtype, device=DEV, seed=21)
    assert ops._C.decode_plan(B, 2, c["block_tables"].shape[1]) == 16
    got = ops.paged_attention_decode(
        c["q"], c["k_cache"], c["v_cache"], c["block_tables"], c["seq_lens"],
        c["scale"])
    out, a = oracle_decode(c["q"], c["k_cache"], c["v_cache"],
                           c["block_tables"], c["seq_lens"], c["scale"])
    assert_within_bound(got, out, a, f"decode/hd{hd}/G7/randn")


@pytest.mark.parametrize("cache_dtype", DTYPES)
def test_decode_g7_rope_fused(cache_dtype, monkeypatch):
    """rope + cache write inside the G = 7 decode kernel: out, fp8 bytes, row
    scales and both caches bit-equal to the two-launch sequence."""
    monkeypatch.delenv("KUBEAI_DECODE_ROPE_FUSED", raising=False)
    torch.manual_seed(97)
    check_fused_equals_two_launches(14, 2, 128, [100, 33, 17, 1],
                                    cache_dtype=cache_dtype, expect_splits=16)


def _generate(seed=11, **kw):
    eng = LLMEngine(EngineConfig(
        model="qwen2-tiny-g7", device=DEV, max_model_len=512,
        num_gpu_blocks=256, seed=seed, **kw))
    # 90 tokens * 7 heads: several waves, past one 16-row tile
    eng.add_request(list(range(10, 100)),
                    SamplingParams(max_tokens=8, ignore_eos=True),
                    request_id="x")
    for _ in range(100):
        for o in eng.step():
            if o.finished:
                return o.output_token_ids
    raise AssertionError("did not finish")


def test_qwen2_g7_engine_gpu():
    a, b = _generate(), _generate()
    assert len(a) == 8 and a == b
    # chunked prefill: 32-token chunks over a growing cached context
    assert len(_generate(max_num_batched_tokens=32)) == 8
