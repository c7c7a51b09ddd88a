"""Grouped int4 MoE experts, CPU side: the torch reference of the grouped
path against MoEMLP's dense expert loop (bit for bit), Int4ExpertGroup, and
the dispatch in MoEMLP.forward."""
import pytest
import torch

from int4_util import random_awq
from kubeai_amd import ops
from kubeai_amd.engine.quant_int4 import (
    Int4ExpertGroup, Int4Linear, Int4Weight, convert_to_int4,
)
from kubeai_amd.models.config import PRESETS
from kubeai_amd.models.llama import MoEMLP


def make_block(E=None, k=None, H=None, inter=None, seed=0, group=128):
    """A MoEMLP with int4 experts; mixtral-tiny's dims unless overridden."""
    import dataclasses

    cfg = PRESETS["mixtral-tiny"]
    over = {}
    if E is not None:
        over["num_local_experts"] = E
    if k is not None:
        over["num_experts_per_tok"] = k
    if H is not None:
        over["hidden_size"] = H
    if inter is not None:
        over["intermediate_size"] = inter
    cfg = dataclasses.replace(cfg, **over)
    torch.manual_seed(seed)
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    convert_to_int4(mlp, group=group)
    return mlp, cfg


def dense_loop(mlp, x):
    """MoEMLP.forward on a CPU tensor is the dense expert loop."""
    assert not x.is_cuda and x.shape[0] <= 256
    return mlp(x)


def route(mlp, x):
    """The routing MoEMLP.forward computes."""
    router = torch.nn.functional.linear(x.float(), mlp.gate.weight.float())
    weights, selected = torch.topk(router, mlp.top_k, dim=-1)
    return selected, torch.softmax(weights, dim=-1).to(x.dtype)


@pytest.fixture(scope="module")
def tiny_block():
    return make_block()


@pytest.mark.parametrize("T", [1, 7, 33, 64])
def test_ref_equals_dense_loop_mixtral_tiny(tiny_block, T):
    mlp, cfg = tiny_block
    assert isinstance(mlp.experts[0].gate_up_proj, Int4Linear)
    torch.manual_seed(T)
    x = torch.randn(T, cfg.hidden_size).to(torch.bfloat16)
    selected, weights = route(mlp, x)
    got = ops.int4_moe_mlp(x, selected, weights, *mlp.int4_groups())
    assert got.shape == x.shape and got.dtype == x.dtype
    assert torch.equal(got, dense_loop(mlp, x))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_ref_equals_dense_loop_e8(k):
    mlp, cfg = make_block(E=8, k=k, H=128, inter=64, seed=k, group=32)
    torch.manual_seed(10 + k)
    x = torch.randn(9, 128).to(torch.bfloat16)
    selected, weights = route(mlp, x)
    if k > 1:
        # topk returns a token's experts by descending logit, which is in
        # descending id order about as often as not: make sure one is
        desc = (selected[:, :-1] > selected[:, 1:]).all(dim=1)
        assert bool(desc.any()), "no token with descending expert ids"
    got = ops.int4_moe_mlp(x, selected, weights, *mlp.int4_groups())
    assert torch.equal(got, dense_loop(mlp, x))


def test_moe_linear_and_combine_refs():
    """The two halves on their own: pair rows are the expert's rows, and the
    combine is the ordered bf16 expression, out-of-range ids skipped."""
    E, k, T, N, K = 4, 2, 5, 32, 64
    ws = [Int4Weight.from_codes(*random_awq(N, K, 32, seed=e)[3]) for e in range(E)]
    group = Int4ExpertGroup(ws)
    torch.manual_seed(0)
    x = torch.randn(T, K).to(torch.bfloat16)
    selected = torch.stack([torch.randperm(E)[:k] for _ in range(T)])
    y = ops.int4_moe_linear(x, selected, group, k)
    assert y.shape == (T * k, N)
    for t in range(T):
        for j in range(k):
            full = ops.int4_linear(x, ws[int(selected[t, j])])
            assert torch.equal(y[t * k + j], full[t])
    xa = torch.randn(T * k, K).to(torch.bfloat16)
    y1 = ops.int4_moe_linear(xa, selected, group, 1)
    for p in range(T * k):
        full = ops.int4_linear(xa, ws[int(selected.view(-1)[p])])
        assert torch.equal(y1[p], full[p])

    w = torch.rand(T, k).to(torch.bfloat16)
    out = ops.moe_combine(y, selected, w, E)
    for t in range(T):
        acc = None
        for j in selected[t].argsort().tolist():
            term = y[t * k + j] * w[t, j]
            acc = term if acc is None else acc + term
        assert torch.equal(out[t], acc)
    bad = selected.clone()
    bad[0, 0] = E + 3
    out_bad = ops.moe_combine(y, bad, w, E)
    assert torch.equal(out_bad[0], y[1] * w[0, 1])
    assert torch.equal(out_bad[1:], out[1:])


def test_expert_group_mismatch_names_expert():
    def w(N, K, g, seed):
        return Int4Weight.from_codes(*random_awq(N, K, g, seed=seed)[3])

    base = [w(32, 128, 32, s) for s in range(3)]
    for bad in (w(32, 256, 32, 9), w(32, 128, 64, 9), w(48, 128, 32, 9)):
        with pytest.raises(ValueError, match="expert 2"):
            Int4ExpertGroup(base[:2] + [bad])
    with pytest.raises(ValueError, match="expert 1"):
        Int4ExpertGroup([base[0], w(16, 128, 32, 9), base[2]])
    g = Int4ExpertGroup(base)
    assert (g.E, g.N, g.K, g.group) == (3, 32, 128, 32)
    assert g.table.dtype == torch.int64 and g.table.shape == (3, 3)
    # the weights themselves, no copy
    assert all(a is b for a, b in zip(g.weights, base))


def table_of(mlp, name):
    return [
        [getattr(ex, name).qweight.data_ptr(), getattr(ex, name).scales.data_ptr(),
         getattr(ex, name).qzeros.data_ptr()]
        for ex in mlp.experts
    ]


def test_group_table_rebuilt_after_move():
    mlp, _ = make_block(seed=3)
    keys = set(mlp.state_dict().keys())
    assert not any("group" in key or "table" in key for key in keys)
    gu, dn = mlp.int4_groups()
    assert gu.table.tolist() == table_of(mlp, "gate_up_proj")
    assert dn.table.tolist() == table_of(mlp, "down_proj")
    old = table_of(mlp, "gate_up_proj")
    keep = [ex.gate_up_proj.qweight for ex in mlp.experts]  # pin old storage
    mlp._apply(lambda t: t.clone())  # what .to(device) does: new buffers
    gu2, dn2 = mlp._int4_groups
    assert gu2 is not gu and dn2 is not dn
    assert gu2.table.tolist() == table_of(mlp, "gate_up_proj") != old
    assert dn2.table.tolist() == table_of(mlp, "down_proj")
    mlp.to("cpu")
    assert mlp._int4_groups[0] is not gu2
    assert set(mlp.state_dict().keys()) == keys
    del keep
    # a replaced buffer is noticed at the next use
    lin = mlp.experts[1].down_proj
    lin.qweight = lin.qweight.clone()
    assert mlp.int4_groups()[1].table.tolist() == table_of(mlp, "down_proj")


def test_float_and_biased_experts_have_no_group():
    import dataclasses

    cfg = PRESETS["mixtral-tiny"]
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    assert mlp.int4_groups() is None
    convert_to_int4(mlp)
    assert mlp.int4_groups() is not None
    mlp.experts[0].down_proj.bias = torch.zeros(cfg.hidden_size)
    assert mlp.refresh_int4_groups() is None
    gelu = MoEMLP(dataclasses.replace(cfg, hidden_act="gelu_pytorch_tanh"))
    convert_to_int4(gelu.to(torch.bfloat16))
    assert gelu.int4_groups() is None


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def test_dispatch_keeps_dense_loop(tiny_block, monkeypatch):
    """The grouped path is for GPU tensors with 1 <= T <= INT4_MOE_T: CPU,
    the switch at 0 and T = 65 all stay on the dense loop."""
    mlp, cfg = tiny_block
    counter = Counter(ops.int4_moe_mlp)
    monkeypatch.setattr(ops, "int4_moe_mlp", counter)
    monkeypatch.setattr(ops, "INT4_MOE_T", 64)
    for T in (1, 64, 65):
        mlp(torch.randn(T, cfg.hidden_size).to(torch.bfloat16))
    monkeypatch.setattr(ops, "INT4_MOE_T", 0)
    mlp(torch.randn(4, cfg.hidden_size).to(torch.bfloat16))
    assert counter.calls == 0
