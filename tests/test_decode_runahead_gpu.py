"""Decode run-ahead on the GPU: the decode_advance kernel against its
reference, the sampler captured in a graph against the eager one, and the
engine with run-ahead on against KUBEAI_DECODE_RUNAHEAD=0, graphs on."""
import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.ops import ref

from runahead_util import ADVANCE_CASES, BS, advance_case, pick_stop, run_traffic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,b_pad", ADVANCE_CASES)
def test_decode_advance_matches_reference(B, b_pad):
    args, exp = advance_case(B, b_pad, device="cuda")
    cpu_args, _ = advance_case(B, b_pad)
    ref.decode_advance(*cpu_args, BS)
    before = [a.clone() for a in args]
    ops.decode_advance(*args, BS)
    torch.cuda.synchronize()
    for name, got, want, r in zip(("ids", "positions", "slots", "seq_lens"),
                                  args[:4], exp, cpu_args[:4]):
        assert torch.equal(r, want), name  # the reference, once more
        assert got.dtype == want.dtype and torch.equal(got.cpu(), want), name
    for got, was in zip(args[4:], before[4:]):
        assert torch.equal(got, was)
    for got, was in zip(args[:4], before[:4]):
        assert torch.equal(got[B:], was[B:])  # pad rows untouched


def test_decode_advance_no_live_rows():
    args, _ = advance_case(5, 8, device="cuda")
    args[6].zero_()  # b_live = 0: an uploaded step
    before = [a.clone() for a in args]
    ops.decode_advance(*args, BS)
    torch.cuda.synchronize()
    for got, was in zip(args, before):
        assert torch.equal(got, was)


@pytest.mark.parametrize("V", [129, 128256])
@pytest.mark.parametrize("B", [1, 40])
@torch.inference_mode()  # as the runner captures: graph state made there is inference state
def test_captured_sampler_equals_eager(B, V):
    """greedy_sample_logprob captured in a graph behind decode_advance, as a
    self-feeding decode graph holds them: several replays over changing
    logits, each byte-equal to the eager call on the same tensor, and the
    advance of the replay after it sees that replay's tokens."""
    gen = torch.Generator(device="cuda").manual_seed(B * 1000 + V)
    draw = lambda: (
        torch.randn(B, V, device="cuda", generator=gen) * 4.0
    ).to(torch.bfloat16)
    logits = draw()
    b_pad = 8 if B == 1 else 64
    args, _ = advance_case(B, b_pad, device="cuda")
    ids, pos, slots, lens, tables, nb, live, _ = args
    nb.fill_(tables.shape[1])  # every row has a block for every position
    pos.fill_(3)
    res = ops.empty_sample_result(B, "cuda")
    tokens_in = torch.zeros(b_pad, dtype=torch.int64, device="cuda")

    def body():
        tokens_in[:B].copy_(res.tokens)
        ops.decode_advance(ids, pos, slots, lens, tables, nb, live, tokens_in, BS)
        ops.greedy_sample_logprob(logits, out=res)

    body()  # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    last = None
    for _ in range(4):
        logits.copy_(draw())
        p0 = pos.clone()
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.greedy_sample_logprob(logits)
        assert eager.tokens.dtype == res.tokens.dtype == torch.int64
        assert torch.equal(res.tokens, eager.tokens)
        for a, b in ((res.logprob, eager.logprob), (res.lse, eager.lse)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        tok, lp = ops.sample_to_host(res)
        assert tok == eager.tokens.tolist() and lp == eager.logprob.tolist()
        assert torch.equal(pos[:B], p0[:B] + 1)
        if last is not None:
            assert torch.equal(ids[:B], last.to(torch.int32))
        last = res.tokens.clone()


@pytest.fixture(scope="module")
def off_plain():
    mp = pytest.MonkeyPatch()
    mp.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    try:
        return run_traffic("cuda")
    finally:
        mp.undo()


def test_engine_equal_with_and_without_runahead(off_plain, monkeypatch):
    stop = pick_stop(off_plain[0])
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    off_steps, off_free, off_stats, off_eng = run_traffic("cuda", stop=stop)
    assert off_eng.runner.enable_graphs and off_eng.runner._graphs
    assert not off_eng.runner.self_feed
    assert off_stats["runahead_enqueued"] == 0
    ended = [o for s in off_steps for o in s if o[0] == stop[0] and o[3]][0]
    assert ended[4] == "stop" and ended[1] == (stop[1],)
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "1")
    on_steps, on_free, on_stats, on_eng = run_traffic("cuda", stop=stop)
    assert on_eng.runner.enable_graphs and on_eng.runner.self_feed
    assert any(isinstance(k, tuple) and k[0] == "feed" for k in on_eng.runner._graphs)
    assert len(on_steps) == len(off_steps)
    for i, (a, b) in enumerate(zip(on_steps, off_steps)):
        assert a == b, f"step {i + 1}"
    assert on_free == off_free
    assert on_stats["runahead_adopted"] >= 1
    assert on_stats["runahead_discarded"] >= 1
    assert on_eng.runner._inflight is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("odd", [
    dict(temperature=0.8, seed=11),
    dict(logit_bias={5: 4.0, 17: -3.0}),
], ids=["temperature", "logit_bias"])
def test_no_runahead_with_host_sampled_request(odd, monkeypatch):
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    off_steps, off_free, _, _ = run_traffic("cuda", odd=odd)
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "1")
    on_steps, on_free, stats, eng = run_traffic("cuda", odd=odd)
    assert eng.runner.self_feed
    assert on_steps == off_steps and on_free == off_free
    last_r2 = max(i for i, s in enumerate(on_steps) if any(o[0] == "r2" for o in s))
    assert last_r2 >= 8
    assert stats["enqueued_by_step"][last_r2] == 0
    torch.cuda.synchronize()
