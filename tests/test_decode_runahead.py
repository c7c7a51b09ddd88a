"""Decode run-ahead without a GPU: the decode_advance reference, and the
engine's run-ahead logic through the reference ops (on a CPU device the
self-feeding decode step runs eagerly; the logic around it is the same)."""
import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.ops import ref

from runahead_util import ADVANCE_CASES, BS, advance_case, pick_stop, run_traffic


@pytest.mark.parametrize("B,b_pad", ADVANCE_CASES)
def test_decode_advance_reference(B, b_pad):
    args, exp = advance_case(B, b_pad)
    before = [a.clone() for a in args]
    ref.decode_advance(*args, BS)
    for name, got, want in zip(("ids", "positions", "slots", "seq_lens"),
                               args[:4], exp):
        assert got.dtype == want.dtype and torch.equal(got, want), name
    for got, was in zip(args[4:], before[4:]):
        assert torch.equal(got, was)  # tables, n_blocks, b_live, tokens
    for got, was in zip(args[:4], before[:4]):
        assert torch.equal(got[B:], was[B:])  # pad rows
    if B >= 5:
        # the case has what it claims: a frozen row, and rows that moved
        assert torch.equal(args[1][4], before[1][4])
        assert int(args[1][1]) % BS == 0 and int(args[1][2]) % BS == 0


def test_decode_advance_dispatches_to_reference():
    args, exp = advance_case(5, 8)
    ops.decode_advance(*args, BS)
    for got, want in zip(args[:4], exp):
        assert torch.equal(got, want)


@pytest.fixture(scope="module")
def off_plain():
    mp = pytest.MonkeyPatch()
    mp.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    try:
        return run_traffic("cpu")
    finally:
        mp.undo()


def test_engine_equal_with_and_without_runahead(off_plain, monkeypatch):
    stop = pick_stop(off_plain[0])
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    off_steps, off_free, off_stats, off_eng = run_traffic("cpu", stop=stop)
    assert not off_eng.runner.self_feed
    assert off_stats["runahead_enqueued"] == 0
    ended = [o for s in off_steps for o in s if o[0] == stop[0] and o[3]][0]
    assert ended[4] == "stop" and ended[1] == (stop[1],)
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "1")
    on_steps, on_free, on_stats, on_eng = run_traffic("cpu", stop=stop)
    assert on_eng.runner.self_feed
    assert len(on_steps) == len(off_steps)
    for i, (a, b) in enumerate(zip(on_steps, off_steps)):
        assert a == b, f"step {i + 1}"
    assert on_free == off_free
    assert on_stats["runahead_adopted"] >= 1
    assert on_stats["runahead_discarded"] >= 1
    assert on_stats["runahead_enqueued"] == (
        on_stats["runahead_adopted"] + on_stats["runahead_discarded"]
    )
    assert on_eng.runner._inflight is None


@pytest.mark.parametrize("odd", [
    dict(temperature=0.8, seed=11),
    dict(logit_bias={5: 4.0, 17: -3.0}),
], ids=["temperature", "logit_bias"])
def test_no_runahead_with_host_sampled_request(odd, monkeypatch):
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "0")
    off_steps, off_free, _, _ = run_traffic("cpu", odd=odd)
    monkeypatch.setenv("KUBEAI_DECODE_RUNAHEAD", "1")
    on_steps, on_free, stats, eng = run_traffic("cpu", odd=odd)
    assert eng.runner.self_feed
    assert on_steps == off_steps and on_free == off_free
    # r2 is in the batch from the first step until it ends: nothing may run
    # ahead of any of those steps (afterwards the batch is all greedy again)
    last_r2 = max(i for i, s in enumerate(on_steps) if any(o[0] == "r2" for o in s))
    assert last_r2 >= 8
    assert stats["enqueued_by_step"][last_r2] == 0
