"""The samplers that also return the token's logprob and the row's logsumexp
(ops.greedy_sample_logprob, ops.gumbel_sample_logprob) and ops.token_logprobs.

Tokens must equal ops.greedy_sample / ops.gumbel_sample exactly. Logprob and
lse are held against an fp64 oracle over the same fp32 logits:

    |lp - lp64| <= 2 * ulp32(max(|lse64|, |x_tok|, 8))

Half an ulp for the add in lse = logf(S) + M, half an ulp for the subtract
x_tok - lse, one ulp for logf(S): S is a sum of positive terms whose relative
error is far below 2^-20, and ulp32(8) = 9.5e-7 bounds what that costs after
the log. The torch fp32 chain the runner used before goes through the same
assertion, which shows the checker accepts it too.

Shapes: B in {1, 5, 40} x V in {31, 129, 1000, 32000, 128256}: V = 31 leaves
splits empty, V = 129 gives chunks smaller than the block, V = 128256 is the
register-resident chunk; V = 131104 (own test) is the first chunk length that
is read twice instead. Row b is of kind (kind0 + b) % 4: randn x 0.3,
randn x 5, randn with a +30 spike, randn x 5 with 30 % of the vocab at -inf.
"""
import functools

import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.ops import ref

BS = (1, 5, 40)
VS = (31, 129, 1000, 32000, 128256)
N_KINDS = 4
SPLITS = 32


def _kind0s(B):
    # every row kind in every shape: a batch shorter than the cycle repeats
    return range(N_KINDS) if B < N_KINDS else (0,)


@functools.lru_cache(maxsize=None)
def _logits(B, V, kind0, device):
    """fp32 [B, V], read-only by convention (shared between tests)."""
    g = torch.Generator().manual_seed(1000 * B + V + 7 * kind0)
    x = torch.randn(B, V, generator=g)
    for b in range(B):
        kind = (kind0 + b) % N_KINDS
        if kind == 0:
            x[b] *= 0.3
        elif kind == 1:
            x[b] *= 5.0
        elif kind == 2:
            x[b, (b * 7919 + 13) % V] += 30.0
        else:
            x[b] *= 5.0
            mask = torch.rand(V, generator=g) < 0.3
            mask[(b * 31 + 5) % V] = False  # never the whole row
            x[b, mask] = float("-inf")
    return x.to(device)


def _ulp32(y):
    """ulp of fp32 at |y| (fp64 tensor of normal magnitudes)."""
    _, e = torch.frexp(y)  # y = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(y), e - 24)


def _oracle(logits, tokens):
    x64 = logits.double()
    lse64 = torch.logsumexp(x64, dim=-1)
    x_tok = x64.gather(1, tokens.view(-1, 1)).squeeze(1)
    return x_tok - lse64, lse64, x_tok


def _assert_within_bound(logits, tokens, logprob, lse, what):
    lp64, lse64, x_tok = _oracle(logits, tokens)
    finite = torch.isfinite(x_tok)
    # a masked token: exactly -inf, never NaN
    assert torch.equal(
        logprob[~finite].double(), torch.full_like(lp64[~finite], float("-inf"))
    ), what
    big = torch.maximum(lse64.abs(), x_tok.abs().where(finite, lse64.abs()))
    bound = 2.0 * _ulp32(big.clamp_min(8.0))
    err_lp = (logprob.double() - lp64).abs()[finite]
    err_lse = (lse.double() - lse64).abs()
    worst_lp = float((err_lp / bound[finite]).max()) if bool(finite.any()) else 0.0
    print(
        f"{what}: logprob err/bound {worst_lp:.3f} "
        f"lse err/bound {float((err_lse / bound).max()):.3f}"
    )
    assert bool((err_lp <= bound[finite]).all()), what
    assert bool((err_lse <= bound).all()), what


def _gumbel_params(B, device):
    temps = torch.tensor([(0.0, 0.7, 1.3)[b % 3] for b in range(B)], device=device)
    seeds = torch.arange(B, dtype=torch.int64, device=device) * 7 + 3
    return temps, seeds


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_greedy_token_logprob_lse(B, V):
    for kind0 in _kind0s(B):
        logits = _logits(B, V, kind0, "cuda")
        res = ops.greedy_sample_logprob(logits)
        assert torch.equal(res.tokens, ops.greedy_sample(logits))
        _assert_within_bound(
            logits, res.tokens, res.logprob, res.lse, f"greedy {B}x{V}/{kind0}"
        )
        # one download carries what the three views hold
        toks, lps = ops.sample_to_host(res)
        assert toks == res.tokens.tolist() and lps == res.logprob.tolist()
        again = ops.greedy_sample_logprob(logits)
        assert torch.equal(again.packed, res.packed)  # bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_gumbel_token_logprob_lse(B, V):
    temps, seeds = _gumbel_params(B, "cuda")
    for kind0 in _kind0s(B):
        logits = _logits(B, V, kind0, "cuda")
        greedy = ops.greedy_sample_logprob(logits)
        for step in (3, 11):
            res = ops.gumbel_sample_logprob(logits, temps, seeds, step)
            assert torch.equal(
                res.tokens, ops.gumbel_sample(logits, temps, seeds, step)
            )
            # logprob and lse are over the raw logits, not the perturbed ones
            _assert_within_bound(
                logits, res.tokens, res.logprob, res.lse,
                f"gumbel {B}x{V}/{kind0} step {step}",
            )
            assert torch.equal(
                res.lse.view(torch.int32), greedy.lse.view(torch.int32)
            )
            again = ops.gumbel_sample_logprob(logits, temps, seeds, step)
            assert torch.equal(again.packed, res.packed)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
def test_ties_lowest_index_wins(V):
    chunk = (V + SPLITS - 1) // SPLITS
    logits = _logits(5, V, 0, "cuda").clone()
    logits[0] = 1.25  # all equal
    # the last logit of split 0 and the first of split 1
    logits[1, chunk - 1] = logits[1, chunk] = 50.0
    # first of the last non-empty split against the last of the one before
    last = ((V - 1) // chunk) * chunk
    logits[2, last - 1] = logits[2, last] = 50.0
    logits[3, V - 1] = logits[3, 0] = 50.0
    want = torch.tensor([0, chunk - 1, last - 1, 0], device="cuda")
    res = ops.greedy_sample_logprob(logits)
    assert torch.equal(res.tokens[:4], want)
    assert torch.equal(res.tokens, ops.greedy_sample(logits))
    temps = torch.zeros(5, device="cuda")
    seeds = torch.arange(5, dtype=torch.int64, device="cuda")
    resg = ops.gumbel_sample_logprob(logits, temps, seeds, 5)
    assert torch.equal(resg.tokens, res.tokens)
    _assert_within_bound(logits, res.tokens, res.logprob, res.lse, f"ties {V}")


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_torch_fp32_chain_meets_the_bound(B, V):
    for kind0 in _kind0s(B):
        logits = _logits(B, V, kind0, "cuda")
        tokens = ops.greedy_sample(logits)
        logprob, lse = ref.token_logprobs(logits, tokens)
        _assert_within_bound(logits, tokens, logprob, lse, f"torch {B}x{V}/{kind0}")


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("B", BS)
def test_token_logprobs(B, V):
    for kind0 in _kind0s(B):
        logits = _logits(B, V, kind0, "cuda")
        fused = ops.greedy_sample_logprob(logits)
        g = torch.Generator().manual_seed(B + V)
        tokens = torch.randint(0, V, (B,), generator=g).cuda()
        tokens[0] = fused.tokens[0]  # the argmax itself
        logprob, lse = ops.token_logprobs(logits, tokens)
        assert not bool(torch.isnan(logprob).any())
        _assert_within_bound(logits, tokens, logprob, lse, f"tokens {B}x{V}/{kind0}")
        # the same arithmetic as the two-stage sampler, to the bit
        assert torch.equal(lse.view(torch.int32), fused.lse.view(torch.int32))
        assert logprob[0].item() == fused.logprob[0].item()
        # a masked-out token in every row that has one: -inf, never NaN
        masked = torch.isinf(logits).any(dim=1).nonzero().flatten().tolist()
        if masked:
            tokens = tokens.clone()
            for b in masked:
                tokens[b] = int(torch.isinf(logits[b]).nonzero()[0])
            logprob, lse = ops.token_logprobs(logits, tokens)
            assert not bool(torch.isnan(logprob).any())
            for b in masked:
                assert float(logprob[b]) == float("-inf")
            _assert_within_bound(
                logits, tokens, logprob, lse, f"masked tokens {B}x{V}/{kind0}"
            )
            assert torch.equal(lse.view(torch.int32), fused.lse.view(torch.int32))
        logprob2, lse2 = ops.token_logprobs(logits, tokens)
        assert torch.equal(logprob2.view(torch.int32), logprob.view(torch.int32))
        assert torch.equal(lse2.view(torch.int32), lse.view(torch.int32))


@pytest.mark.gpu
def test_chunk_longer_than_the_registers():
    # 32 * 256 * 16 = 131072 logits fit the register-resident sweep; one more
    # vocab entry per split and the chunk is read twice
    B, V = 3, 131104
    logits = _logits(B, V, 1, "cuda")
    temps, seeds = _gumbel_params(B, "cuda")
    res = ops.greedy_sample_logprob(logits)
    assert torch.equal(res.tokens, ops.greedy_sample(logits))
    _assert_within_bound(logits, res.tokens, res.logprob, res.lse, "greedy long")
    resg = ops.gumbel_sample_logprob(logits, temps, seeds, 4)
    assert torch.equal(resg.tokens, ops.gumbel_sample(logits, temps, seeds, 4))
    _assert_within_bound(logits, resg.tokens, resg.logprob, resg.lse, "gumbel long")
    _, lse = ops.token_logprobs(logits, res.tokens)
    assert torch.equal(lse.view(torch.int32), res.lse.view(torch.int32))
    assert torch.equal(ops.greedy_sample_logprob(logits).packed, res.packed)


@pytest.mark.parametrize("V", (31, 1000, 128256))
def test_cpu_fallbacks_meet_the_bound(V):
    B = 5
    logits = _logits(B, V, 0, "cpu")
    res = ops.greedy_sample_logprob(logits)
    assert torch.equal(res.tokens, logits.argmax(-1))
    _assert_within_bound(logits, res.tokens, res.logprob, res.lse, f"cpu greedy {V}")
    assert ops.sample_to_host(res) == (res.tokens.tolist(), res.logprob.tolist())
    # today's torch expressions, bit for bit
    lse = torch.logsumexp(logits, dim=-1)
    chosen = logits.gather(1, res.tokens.view(-1, 1)).squeeze(1)
    assert torch.equal(res.logprob, chosen - lse) and torch.equal(res.lse, lse)
    temps, seeds = _gumbel_params(B, "cpu")
    resg = ops.gumbel_sample_logprob(logits, temps, seeds, 3)
    assert torch.equal(resg.tokens, ops.gumbel_sample(logits, temps, seeds, 3))
    _assert_within_bound(logits, resg.tokens, resg.logprob, resg.lse, f"cpu gumbel {V}")
    g = torch.Generator().manual_seed(V)
    tokens = torch.randint(0, V, (B,), generator=g)
    logprob, lse2 = ops.token_logprobs(logits, tokens)
    _assert_within_bound(logits, tokens, logprob, lse2, f"cpu tokens {V}")
