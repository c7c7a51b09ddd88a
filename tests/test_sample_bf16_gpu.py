"""The samplers on bf16 logits against the same calls on logits.float().

bf16 widens to fp32 exactly and the kernels compute on the widened value, so
token, logprob and lse must be bit-equal, not close.

V = 31 and 129 are odd: every other bf16 row starts 2 B aligned, and the 32
chunks are of 1 and 5 logits with empty ones behind them. 32000 and 128256
are the llama vocabularies (register-resident chunks of 1000 and 4008).
"""
import pytest
import torch

import kubeai_amd.ops as ops

pytestmark = pytest.mark.gpu

SHAPES = [(B, V) for B in (1, 5, 40) for V in (31, 129, 32000, 128256)]

_LOGITS = {}


def _logits(B, V):
    """(bf16 logits, their fp32 widening), shared and never written to."""
    if (B, V) not in _LOGITS:
        gen = torch.Generator().manual_seed(B * 1_000_003 + V)
        x = (4.0 * torch.randn(B, V, generator=gen)).to(torch.bfloat16)
        # ties for the argmax in row 0: the lowest index has to win in both
        top = x[0].max()
        x[0, V // 3] = top
        x[0, V - 1] = top
        x = x.cuda()
        _LOGITS[(B, V)] = (x, x.float())
    return _LOGITS[(B, V)]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("B,V", SHAPES)
def test_greedy(B, V):
    lb, lf = _logits(B, V)
    a, b = ops.greedy_sample_logprob(lb), ops.greedy_sample_logprob(lf)
    _same(a.tokens, b.tokens)
    _same(a.logprob, b.logprob)
    _same(a.lse, b.lse)
    _same(ops.greedy_sample(lb), b.tokens)
    assert int(a.tokens[0]) <= V // 3


@pytest.mark.parametrize("B,V", SHAPES)
def test_gumbel(B, V):
    lb, lf = _logits(B, V)
    temps = torch.linspace(0.5, 1.5, B, device="cuda")
    temps[0] = 0.0  # a greedy row among sampled ones
    seeds = torch.arange(B, dtype=torch.int64, device="cuda") * 7919 + 11
    a = ops.gumbel_sample_logprob(lb, temps, seeds, 5)
    b = ops.gumbel_sample_logprob(lf, temps, seeds, 5)
    _same(a.tokens, b.tokens)
    _same(a.logprob, b.logprob)
    _same(a.lse, b.lse)
    _same(ops.gumbel_sample(lb, temps, seeds, 5), b.tokens)


@pytest.mark.parametrize("B,V", SHAPES)
def test_token_logprobs(B, V):
    lb, lf = _logits(B, V)
    gen = torch.Generator().manual_seed(V + B)
    tokens = torch.randint(0, V, (B,), generator=gen).cuda()
    tokens[0] = V - 1
    lp_a, lse_a = ops.token_logprobs(lb, tokens)
    lp_b, lse_b = ops.token_logprobs(lf, tokens)
    _same(lp_a, lp_b)
    _same(lse_a, lse_b)
    # and the sampler pair's lse, as for fp32 logits
    _same(lse_a, ops.greedy_sample_logprob(lb).lse)
