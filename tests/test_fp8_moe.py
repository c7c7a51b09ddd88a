"""Grouped fp8 MoE experts, CPU side: the torch reference of the grouped path
against a per-pair loop of Fp8Linear.forward_quantized, Fp8ExpertGroup, the
KUBEAI_FP8_MOE_T switch and the dispatch in MoEMLP.forward."""
import dataclasses

import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.engine.quant import Fp8ExpertGroup, Fp8Linear, convert_to_fp8
from kubeai_amd.models.config import PRESETS
from kubeai_amd.models.llama import MoEMLP
from kubeai_amd.ops import ref


def make_block(seed=0, **over):
    """A MoEMLP with fp8 experts; mixtral-tiny's dims unless overridden."""
    cfg = dataclasses.replace(PRESETS["mixtral-tiny"], **over)
    torch.manual_seed(seed)
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    convert_to_fp8(mlp)
    return mlp, cfg


def route(mlp, x):
    """The routing MoEMLP.forward computes."""
    router = torch.nn.functional.linear(x.float(), mlp.gate.weight.float())
    weights, selected = torch.topk(router, mlp.top_k, dim=-1)
    return selected, torch.softmax(weights, dim=-1).to(x.dtype)


def random_linears(E, N, K, seed):
    torch.manual_seed(seed)
    return [Fp8Linear(torch.randn(N, K).to(torch.bfloat16)) for _ in range(E)]


@pytest.fixture(scope="module")
def tiny_block():
    return make_block()


def test_ref_linear_is_forward_quantized_per_pair():
    E, k, T, N, K = 4, 2, 5, 32, 64
    linears = random_linears(E, N, K, seed=0)
    group = Fp8ExpertGroup(linears)
    assert (group.E, group.N, group.K) == (E, N, K)
    assert group.table.dtype == torch.int64 and group.table.shape == (E, 2)
    assert group.table.tolist() == [
        [lin.weight_fp8.data_ptr(), lin.weight_scale.data_ptr()]
        for lin in linears
    ]
    assert all(a is b for a, b in zip(group.linears, linears))  # no copy
    selected = torch.stack([torch.randperm(E)[:k] for _ in range(T)])
    xq, xs = ref.quant_fp8(torch.randn(T, K).to(torch.bfloat16))
    pairs = [(lin.weight_fp8, lin.weight_scale) for lin in linears]
    y = ref.fp8_moe_linear(xq, xs, selected, pairs, k)
    assert y.shape == (T * k, N) and y.dtype == torch.bfloat16
    assert torch.equal(y, ops.fp8_moe_linear(xq, xs, selected, group, k))
    for t in range(T):
        for j in range(k):
            full = linears[int(selected[t, j])].forward_quantized(xq, xs)
            assert torch.equal(y[t * k + j], full[t])
    aq, a_s = ref.quant_fp8(torch.randn(T * k, K).to(torch.bfloat16))
    out = torch.empty(T * k, N, dtype=torch.bfloat16)
    y1 = ops.fp8_moe_linear(aq, a_s, selected, group, 1, out=out)
    assert y1 is out
    for p in range(T * k):
        full = linears[int(selected.view(-1)[p])].forward_quantized(aq, a_s)
        assert torch.equal(y1[p], full[p])


@pytest.mark.parametrize("T", [1, 7, 33])
def test_ref_block_is_the_per_pair_loop(tiny_block, T):
    mlp, cfg = tiny_block
    k = mlp.top_k
    assert isinstance(mlp.experts[0].gate_up_proj, Fp8Linear)
    torch.manual_seed(T)
    x = torch.randn(T, cfg.hidden_size).to(torch.bfloat16)
    selected, weights = route(mlp, x)
    got = ops.fp8_moe_mlp(x, selected, weights, *mlp.fp8_groups())
    assert got.shape == x.shape and got.dtype == x.dtype
    xq, xs = ops.quant_fp8(x)
    # each expert on all rows, as forward_quantized is called by the dense loop
    per_expert = []
    for ex in mlp.experts:
        a8, a_s = ops.silu_and_mul_fp8(ex.gate_up_proj.forward_quantized(xq, xs))
        per_expert.append(ex.down_proj.forward_quantized(a8, a_s))
    y = torch.stack([
        per_expert[int(selected[t, j])][t] for t in range(T) for j in range(k)
    ])
    assert torch.equal(got, ref.moe_combine(y, selected, weights, len(mlp.experts)))
    # ... which is the dense loop itself
    assert torch.equal(got, mlp(x))


def test_expert_group_errors_name_the_fault():
    base = random_linears(3, 32, 64, seed=1)
    with pytest.raises(ValueError, match="no experts"):
        Fp8ExpertGroup([])
    with pytest.raises(ValueError, match="expert 1 is a Linear"):
        Fp8ExpertGroup([base[0], torch.nn.Linear(64, 32, bias=False), base[2]])
    biased = Fp8Linear(torch.randn(32, 64).to(torch.bfloat16), torch.zeros(32))
    with pytest.raises(ValueError, match="expert 2 has a bias"):
        Fp8ExpertGroup(base[:2] + [biased])
    for shape in ((48, 64), (32, 128)):
        other = Fp8Linear(torch.randn(*shape).to(torch.bfloat16))
        with pytest.raises(ValueError, match=r"expert 2 is \[\d+, \d+\]"):
            Fp8ExpertGroup(base[:2] + [other])
    meta = Fp8Linear(torch.randn(32, 64).to(torch.bfloat16)).to("meta")
    with pytest.raises(ValueError, match="expert 1 is on meta"):
        Fp8ExpertGroup([base[0], meta])
    strided = Fp8Linear(torch.randn(32, 64).to(torch.bfloat16))
    strided.weight_fp8 = (
        torch.zeros(32, 128).to(torch.float8_e4m3fn)[:, ::2]
    )
    with pytest.raises(ValueError, match="expert 0's weight.*contiguous"):
        Fp8ExpertGroup([strided])


def table_of(mlp, name):
    return [
        [getattr(ex, name).weight_fp8.data_ptr(),
         getattr(ex, name).weight_scale.data_ptr()]
        for ex in mlp.experts
    ]


def test_group_table_built_at_convert_and_rebuilt_after_move():
    mlp, _ = make_block(seed=3)
    keys = set(mlp.state_dict().keys())
    assert not any("group" in key or "table" in key for key in keys)
    assert mlp._fp8_groups is not None, "convert_to_fp8 builds the groups"
    assert mlp.int4_groups() is None
    gu, dn = mlp.fp8_groups()
    assert gu.table.tolist() == table_of(mlp, "gate_up_proj")
    assert dn.table.tolist() == table_of(mlp, "down_proj")
    assert gu.holds([ex.gate_up_proj for ex in mlp.experts])
    assert not gu.holds([ex.down_proj for ex in mlp.experts])
    old = table_of(mlp, "gate_up_proj")
    keep = [ex.gate_up_proj.weight_fp8 for ex in mlp.experts]  # pin old storage
    mlp._apply(lambda t: t.clone())  # what .to(device) does: new buffers
    gu2, dn2 = mlp._fp8_groups
    assert gu2 is not gu and dn2 is not dn
    assert gu2.table.tolist() == table_of(mlp, "gate_up_proj") != old
    assert dn2.table.tolist() == table_of(mlp, "down_proj")
    assert set(mlp.state_dict().keys()) == keys
    del keep
    # a replaced buffer is noticed at the next use
    lin = mlp.experts[1].down_proj
    lin.weight_fp8 = lin.weight_fp8.clone()
    assert mlp.fp8_groups()[1].table.tolist() == table_of(mlp, "down_proj")


def test_float_biased_and_gelu_experts_have_no_group():
    cfg = PRESETS["mixtral-tiny"]
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    assert mlp.fp8_groups() is None
    convert_to_fp8(mlp)
    assert mlp.fp8_groups() is not None
    mlp.experts[0].down_proj.bias = torch.zeros(cfg.hidden_size)
    assert mlp.refresh_fp8_groups() is None
    gelu = MoEMLP(dataclasses.replace(cfg, hidden_act="gelu_pytorch_tanh"))
    convert_to_fp8(gelu.to(torch.bfloat16))
    assert gelu.fp8_groups() is None


@pytest.mark.parametrize("value, want", [
    (None, 0), ("64", 64), ("999", 64), ("0", 0), ("16", 16), ("-3", 0),
    ("many", 0),
])
def test_fp8_moe_t_is_read_at_call_time(monkeypatch, value, want):
    if value is None:
        monkeypatch.delenv("KUBEAI_FP8_MOE_T", raising=False)
    else:
        monkeypatch.setenv("KUBEAI_FP8_MOE_T", value)
    assert ops.fp8_moe_t() == want


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def test_cpu_never_takes_the_branch(tiny_block, monkeypatch):
    mlp, cfg = tiny_block
    counter = Counter(ops.fp8_moe_mlp)
    monkeypatch.setattr(ops, "fp8_moe_mlp", counter)
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    assert ops.fp8_moe_t() == 64
    for T in (1, 64, 65):
        mlp(torch.randn(T, cfg.hidden_size).to(torch.bfloat16))
    monkeypatch.delenv("KUBEAI_FP8_MOE_T")
    mlp(torch.randn(4, cfg.hidden_size).to(torch.bfloat16))
    assert counter.calls == 0
