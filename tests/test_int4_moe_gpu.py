"""Grouped int4 MoE experts on the GPU: int4_moe_gemm's pair rows against the
served int4_gemm kernel (bit for bit), skewed routings, the combine, the whole
block against MoEMLP's dense expert loop, graph replay under a changed
routing, the launch plan, host errors and the engine end to end."""
import dataclasses

import pytest
import torch

from int4_util import generate, random_awq
from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_int4 import (
    Int4ExpertGroup, Int4Linear, Int4Weight, convert_to_int4,
)
from kubeai_amd.models.config import PRESETS
from kubeai_amd.models.llama import MoEMLP

pytestmark = pytest.mark.gpu

DEV = "cuda"
E, TOPK = 4, 2
# 3 chunks over the 8-wave split with group boundaries inside a chunk, and a
# ragged last chunk
SHAPES = [(48, 384, 32), (48, 384, 128), (16, 160, 32)]
SENTINEL = 7.0


def bits(t):
    return t.contiguous().view(torch.int16)


def random_routing(T, n_experts, k, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randperm(n_experts, generator=gen)[:k] for _ in range(T)]
    return torch.stack(rows).to(torch.int64)


@pytest.fixture(scope="module")
def experts():
    """shape -> (CPU weights, GPU weights, GPU group); built once."""
    out = {}
    for N, K, g in SHAPES:
        cpu = [
            Int4Weight.from_codes(*random_awq(N, K, g, seed=100 * e + g)[3])
            for e in range(E)
        ]
        dev = [w.to(DEV) for w in cpu]
        out[(N, K, g)] = (cpu, dev, Int4ExpertGroup(dev))
    return out


def assert_plan(N, T, n_experts=E, k=TOPK, nt=1):
    from kubeai_amd import _C

    assert _C.int4_moe_plan(N, T, n_experts, k) == ((T + 15) // 16, nt)


def assert_pair_rows(y, x, selected, dev_weights, row_div):
    """Every pair row of y is int4_linear's row for that pair's input row and
    expert, as bit patterns. Returns the number of pairs checked."""
    flat = selected.view(-1)
    seen = 0
    for e, w in enumerate(dev_weights):
        pairs = (flat == e).nonzero().view(-1)
        if pairs.numel() == 0:
            continue
        ref = ops.int4_linear(x[pairs // row_div], w)
        assert torch.equal(bits(y[pairs]), bits(ref)), f"expert {e}"
        seen += pairs.numel()
    return seen


# --------------------------------------------------- 1. rows = served kernel
@pytest.mark.parametrize("T", [1, 5, 17, 33, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_rows_bit_equal(experts, shape, T):
    N, K, g = shape
    _, dev, group = experts[shape]
    assert_plan(N, T)
    selected = random_routing(T, E, TOPK, seed=T + g).to(DEV)
    torch.manual_seed(T)
    x = torch.randn(T, K).to(torch.bfloat16).to(DEV)
    y = ops.int4_moe_linear(x, selected, group, TOPK)
    assert y.shape == (T * TOPK, N) and y.dtype == torch.bfloat16
    assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK
    xa = torch.randn(T * TOPK, K).to(torch.bfloat16).to(DEV)
    y1 = ops.int4_moe_linear(xa, selected, group, 1)
    assert assert_pair_rows(y1, xa, selected, dev, 1) == T * TOPK


def wide_experts(N, K, g):
    gen = torch.Generator().manual_seed(N)
    cpu = [
        Int4Weight.from_codes(
            torch.randint(0, 16, (N, K), generator=gen, dtype=torch.uint8),
            torch.randint(0, 16, (N, K // g), generator=gen, dtype=torch.uint8),
            (torch.rand(N, K // g, generator=gen) * 0.02 + 0.001).half(),
        )
        for _ in range(E)
    ]
    dev = [w.to(DEV) for w in cpu]
    return dev, Int4ExpertGroup(dev)


def test_wide_workgroups_forced():
    """Workgroups of 2 and 4 column tiles at every row-tile count, asked for
    through n_tiles (N = 64 is four tiles; the plan itself takes 1 there)."""
    from kubeai_amd import _C

    N, K, g = 64, 384, 64
    dev, group = wide_experts(N, K, g)
    for T in (5, 17, 33, 64):
        selected = random_routing(T, E, TOPK, seed=T).to(DEV)
        torch.manual_seed(T)
        x = torch.randn(T, K).to(torch.bfloat16).to(DEV)
        for nt in (1, 2, 4):
            if T > 48 and nt == 4:
                continue
            y = torch.full((T * TOPK, N), SENTINEL, dtype=torch.bfloat16,
                           device=DEV)
            _C.int4_moe_gemm(y, x, selected, group.table, TOPK, E, N, K, g, nt)
            assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK, nt
    y = torch.empty(2 * TOPK, N, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="4 x 4"):
        _C.int4_moe_gemm(y.new_empty(128, N), x, selected, group.table, TOPK,
                         E, N, K, g, 4)
    with pytest.raises(RuntimeError, match="column tiles"):
        _C.int4_moe_gemm(y, x[:2], selected[:2], group.table, TOPK, E, N, K, g, 3)


def test_wide_workgroups_planned():
    """The smallest N (a multiple of 64) at which the plan itself takes 4
    column tiles for E = 4, k = 2, T = 17: two row tiles by four column
    tiles, with the needle, which is exact in every column."""
    N, K, g, T = 7232, 384, 128, 17
    assert_plan(N, T, nt=4)
    assert_plan(N - 64, T, nt=2)
    dev, group = wide_experts(N, K, g)
    selected = random_routing(T, E, TOPK, seed=3).to(DEV)
    x = torch.zeros(T, K, dtype=torch.bfloat16, device=DEV)
    x[torch.arange(T), 100 + torch.arange(T)] = 1.0
    y = ops.int4_moe_linear(x, selected, group, TOPK)
    assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK
    deq = ops.int4_dequant(dev[1])
    pairs = (selected.view(-1) == 1).nonzero().view(-1)
    assert pairs.numel() > 0
    assert torch.equal(y[pairs], deq[:, 100 + pairs // TOPK].t())


# ------------------------------------------------------- 2. skewed routing
def skewed(second):
    """T = 64, every token's first choice expert 2, second choices given as
    (expert, count) runs."""
    col = torch.cat([torch.full((n,), e) for e, n in second])
    assert col.numel() == 64
    return torch.stack([torch.full((64,), 2), col], dim=1).to(torch.int64)


@pytest.mark.parametrize("second", [
    # expert 2 takes 64 pairs (all four row tiles); 16 and 17 pairs sit on
    # either side of a tile boundary
    [(0, 16), (1, 17), (3, 31)],
    # expert 3 takes none
    [(0, 16), (1, 48)],
    [(3, 1), (0, 63)],
])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_skewed_routing(experts, shape, second):
    N, K, g = shape
    _, dev, group = experts[shape]
    T = 64
    assert_plan(N, T)
    selected = skewed(second).to(DEV)
    torch.manual_seed(g)
    x = torch.randn(T, K).to(torch.bfloat16).to(DEV)
    buf = torch.full((T * TOPK + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = ops.int4_moe_linear(x, selected, group, TOPK, out=buf[: T * TOPK])
    assert y.data_ptr() == buf.data_ptr()
    assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK
    # random rows never reproduce the sentinel in all N columns
    assert not bool((y == SENTINEL).all(dim=1).any())
    assert bool((buf[T * TOPK] == SENTINEL).all())


def test_any_routing_stays_in_bounds(experts):
    """Ids outside [0, E) belong to no workgroup: their rows are not written,
    the others are right. A token that names one expert twice (invalid: its
    results are unspecified) still writes nothing outside y."""
    shape = SHAPES[0]
    N, K, g = shape
    _, dev, group = experts[shape]
    T = 64
    selected = random_routing(T, E, TOPK, seed=9)
    selected[3, 0], selected[10, 1], selected[40, 0] = -1, E, 2**40 + 1
    selected = selected.to(DEV)
    torch.manual_seed(0)
    x = torch.randn(T, K).to(torch.bfloat16).to(DEV)
    buf = torch.full((T * TOPK + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = ops.int4_moe_linear(x, selected, group, TOPK, out=buf[: T * TOPK])
    assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK - 3
    for p in (3 * TOPK, 10 * TOPK + 1, 40 * TOPK):
        assert bool((y[p] == SENTINEL).all())
    assert bool((buf[T * TOPK] == SENTINEL).all())

    twice = torch.zeros(T, TOPK, dtype=torch.int64, device=DEV)  # 128 > 64
    buf.fill_(SENTINEL)
    ops.int4_moe_linear(x, twice, group, TOPK, out=buf[: T * TOPK])
    torch.cuda.synchronize()
    assert bool((buf[T * TOPK] == SENTINEL).all())


# ----------------------------------------------------------- 3. the needle
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_identity_needle(experts, shape):
    """x[t] is one-hot at k = t, so y[t*k + j, n] is W_e[n, t] exactly for
    e = selected[t, j]: a wrong row gather, expert pointer or pair index
    shows as a wrong weight."""
    N, K, g = shape
    cpu, _, group = experts[shape]
    T = 33
    selected = random_routing(T, E, TOPK, seed=g)
    x = torch.zeros(T, K, dtype=torch.bfloat16)
    x[torch.arange(T), torch.arange(T)] = 1.0
    y = ops.int4_moe_linear(x.to(DEV), selected.to(DEV), group, TOPK).cpu()
    deq = torch.stack([w.dequant() for w in cpu])  # [E, N, K]
    for t in range(T):
        for j in range(TOPK):
            want = deq[int(selected[t, j]), :, t]
            assert torch.equal(y[t * TOPK + j], want), (t, j)


def test_row_strided_x(experts):
    shape = SHAPES[1]
    N, K, g = shape
    _, dev, group = experts[shape]
    T = 17
    selected = random_routing(T, E, TOPK, seed=1).to(DEV)
    torch.manual_seed(1)
    big = torch.randn(T, 3 * K).to(torch.bfloat16).to(DEV)
    x = big[:, K : 2 * K]
    assert not x.is_contiguous()
    y = ops.int4_moe_linear(x, selected, group, TOPK)
    assert torch.equal(
        bits(y), bits(ops.int4_moe_linear(x.contiguous(), selected, group, TOPK))
    )
    assert assert_pair_rows(y, x, selected, dev, TOPK) == T * TOPK


# -------------------------------------------------------------- 4. combine
@pytest.mark.parametrize("H", [256, 4096])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_combine_is_the_ordered_bf16_sum(k, H):
    T, n_experts = 7, 8
    selected = random_routing(T, n_experts, k, seed=k).to(DEV)
    torch.manual_seed(H + k)
    scale = 10.0 ** (torch.rand(T * k, 1) * 5.0 - 3.0)  # 1e-3 .. 1e2
    y = (torch.randn(T * k, H) * scale).to(torch.bfloat16).to(DEV)
    y[0, :8] = 0.0
    w = torch.softmax(torch.randn(T, k), dim=-1).to(torch.bfloat16).to(DEV)
    got = ops.moe_combine(y, selected, w, n_experts)
    assert got.shape == (T, H) and got.dtype == torch.bfloat16
    order = selected.argsort(dim=1)
    rows = torch.arange(T, device=DEV)
    acc = None
    for j in range(k):
        idx = order[:, j]
        term = y.view(T, k, H)[rows, idx] * w[rows, idx].unsqueeze(1)
        acc = term if acc is None else acc + term
    assert torch.equal(got, acc)


# ---------------------------------------------------------------- 5. block
def make_block(n_experts, k, H, inter, seed):
    cfg = dataclasses.replace(
        PRESETS["mixtral-tiny"], num_local_experts=n_experts,
        num_experts_per_tok=k, hidden_size=H, intermediate_size=inter,
    )
    torch.manual_seed(seed)
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    convert_to_int4(mlp)
    return mlp.to(DEV)


def route(mlp, x):
    router = torch.nn.functional.linear(x.float(), mlp.gate.weight.float())
    weights, selected = torch.topk(router, mlp.top_k, dim=-1)
    return selected, torch.softmax(weights, dim=-1).to(x.dtype)


@pytest.fixture(scope="module")
def blocks():
    return {
        "tiny": make_block(4, 2, 256, 512, seed=0),
        "e8": make_block(8, 2, 512, 384, seed=1),
    }


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


@pytest.mark.parametrize("T", [1, 7, 33, 64])
@pytest.mark.parametrize("name", ["tiny", "e8"])
def test_block_equals_dense_loop(blocks, name, T, monkeypatch):
    mlp = blocks[name]
    assert isinstance(mlp.experts[0].down_proj, Int4Linear)
    gu, dn = mlp.int4_groups()
    assert gu.table.is_cuda and gu.table.tolist() == [
        [ex.gate_up_proj.qweight.data_ptr(), ex.gate_up_proj.scales.data_ptr(),
         ex.gate_up_proj.qzeros.data_ptr()] for ex in mlp.experts
    ]
    torch.manual_seed(T)
    x = torch.randn(T, mlp.gate.in_features).to(torch.bfloat16).to(DEV)
    selected, weights = route(mlp, x)
    got = ops.int4_moe_mlp(x, selected, weights, gu, dn)
    counter = Counter(ops.int4_moe_mlp)
    monkeypatch.setattr(ops, "int4_moe_mlp", counter)
    monkeypatch.setattr(ops, "INT4_MOE_T", 64)
    through_module = mlp(x)
    assert counter.calls == 1
    monkeypatch.setattr(ops, "INT4_MOE_T", 0)
    dense = mlp(x)
    assert counter.calls == 1, "the switch at 0 must keep the dense loop"
    assert torch.equal(got, dense)
    assert torch.equal(through_module, dense)


def test_module_dispatch_limits(blocks, monkeypatch):
    mlp = blocks["tiny"]
    counter = Counter(ops.int4_moe_mlp)
    monkeypatch.setattr(ops, "int4_moe_mlp", counter)
    monkeypatch.setattr(ops, "INT4_MOE_T", 64)
    x = torch.randn(65, 256).to(torch.bfloat16).to(DEV)
    mlp(x)
    assert counter.calls == 0
    mlp(x[:64])
    assert counter.calls == 1
    monkeypatch.setattr(ops, "INT4_MOE_T", 16)
    mlp(x[:17])
    assert counter.calls == 1
    mlp(x[:16])
    assert counter.calls == 2


# ---------------------------------------------------------- 6. graph replay
def test_routing_is_read_at_replay(blocks):
    mlp = blocks["e8"]
    gu, dn = mlp.int4_groups()
    T, H, n_experts = 17, 512, 8
    torch.manual_seed(5)
    cases = []
    for seed in (1, 2):
        x = torch.randn(T, H).to(torch.bfloat16).to(DEV)
        selected = random_routing(T, n_experts, 2, seed).to(DEV)
        w = torch.softmax(torch.randn(T, 2), dim=-1).to(torch.bfloat16).to(DEV)
        cases.append((x, selected, w, ops.int4_moe_mlp(x, selected, w, gu, dn)))
    assert not torch.equal(cases[0][1], cases[1][1])
    assert not torch.equal(cases[0][3], cases[1][3])
    xs, sels, ws = (t.clone() for t in cases[0][:3])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.int4_moe_mlp(xs, sels, ws, gu, dn)
    for x, selected, w, eager in (cases[1], cases[0], cases[1]):
        xs.copy_(x)
        sels.copy_(selected)
        ws.copy_(w)
        results = []
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            results.append(out.clone())
        assert torch.equal(results[0], eager)
        assert torch.equal(bits(results[0]), bits(results[1]))


# ------------------------------------------------------------------ 7. plan
def test_plan():
    """(row tiles, column tiles per workgroup): ceil(T / 16) row tiles, and
    the widest of 4, 2, 1 column tiles that divides N / 16 and leaves the
    E * (1 - (1 - k/E)^T) experts expected to be active at least 450
    workgroups, 4 x 4 excluded."""
    from kubeai_amd import _C

    for N, _, _ in SHAPES:
        for T in (1, 5, 17, 33, 64):
            assert _C.int4_moe_plan(N, T, E, TOPK) == ((T + 15) // 16, 1)
    for N, T, want in [
        (28672, 1, (1, 4)), (28672, 16, (1, 4)), (28672, 64, (4, 2)),
        (4096, 1, (1, 1)), (4096, 16, (1, 4)), (4096, 64, (4, 2)),
        # what the floor was read from: 2 and 3.5 expected experts x 128
        # column blocks lost, 7.2 x 64 gained
        (4096, 2, (1, 1)), (4096, 4, (1, 2)), (4096, 8, (1, 4)),
    ]:
        assert _C.int4_moe_plan(N, T, 8, 2) == want, (N, T)
    # T = 16: 7.92 experts expected, so 57 column blocks reach 450, 56 do not
    assert _C.int4_moe_plan(57 * 64, 16, 8, 2) == (1, 4)
    assert _C.int4_moe_plan(56 * 64, 16, 8, 2) == (1, 2)
    assert _C.int4_moe_plan(127 * 16, 16, 8, 2) == (1, 1)  # odd tile count
    assert _C.int4_moe_plan(16384, 48, 8, 2) == (3, 4)
    assert _C.int4_moe_plan(16384, 49, 8, 2) == (4, 2)
    assert _C.int4_moe_plan(496 * 16, 4, 8, 1) == (1, 2)   # 3.3 experts x 248


# ----------------------------------------------------------- 8. host errors
def test_host_errors(experts):
    from kubeai_amd import _C

    shape = SHAPES[0]
    N, K, g = shape
    group = experts[shape][2]

    def call(x, selected, row_div, y_rows=None):
        n = selected.numel() if y_rows is None else y_rows
        y = torch.full((n, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
        _C.int4_moe_gemm(y, x, selected, group.table, row_div, E, N, K, g)
        return y

    def xrows(n):
        return torch.zeros(n, K, dtype=torch.bfloat16, device=DEV)

    def sel(T, k):
        return torch.zeros(T, k, dtype=torch.int64, device=DEV)

    call(xrows(4), random_routing(4, E, 2, 0).to(DEV), 2)  # the valid form
    with pytest.raises(RuntimeError, match=r"T in \[1, 64\]"):
        call(xrows(65), sel(65, 2), 2)
    with pytest.raises(RuntimeError, match=r"k in \[1, 8\]"):
        call(xrows(4), sel(4, 9), 9)
    wide = torch.zeros(4, K + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(wide[:, 1 : K + 1], sel(4, 2), 2)
    with pytest.raises(RuntimeError, match="rows"):
        call(xrows(5), sel(4, 2), 2)
    with pytest.raises(RuntimeError, match="rows"):
        call(xrows(4), sel(4, 2), 1)
    with pytest.raises(RuntimeError):
        call(xrows(4), sel(4, 2).to(torch.int32), 2)
    with pytest.raises(RuntimeError):
        call(xrows(4).float(), sel(4, 2), 2)
    with pytest.raises(RuntimeError):
        call(xrows(4), sel(4, 2), 2, y_rows=7)
    with pytest.raises(RuntimeError):
        ops.int4_moe_linear(xrows(4), sel(4, 2), group, 2,
                            out=torch.zeros(8, N, device=DEV))  # fp32 out


# --------------------------------------------------------------- 9. engine
def test_engine_grouped_path_tokens(monkeypatch):
    def engine():
        return LLMEngine(
            EngineConfig(model="mixtral-tiny", device=DEV, num_gpu_blocks=128,
                         max_model_len=512, seed=3, quantization="int4")
        )

    counter = Counter(ops.int4_moe_mlp)
    monkeypatch.setattr(ops, "int4_moe_mlp", counter)
    default_t = ops.INT4_MOE_T
    assert default_t >= 1
    prompt = list(range(10, 60))

    eng = engine()
    assert eng.runner.enable_graphs
    mlp = eng.runner.model.layers[0].mlp
    assert isinstance(mlp.experts[0].gate_up_proj, Int4Linear)
    assert mlp.int4_groups() is not None and mlp.int4_groups()[0].table.is_cuda
    grouped = generate(eng, prompt, 16)
    assert len(grouped) == 16
    assert eng.runner._graphs, "decode did not go through a captured graph"
    assert counter.calls > 0, "the grouped path did not run"
    del eng

    calls = counter.calls
    monkeypatch.setattr(ops, "INT4_MOE_T", 0)
    dense = engine()
    assert generate(dense, prompt, 16) == grouped
    assert counter.calls == calls, "the switch at 0 still took the grouped path"
    del dense

    monkeypatch.setattr(ops, "INT4_MOE_T", default_t)
    monkeypatch.setenv("KUBEAI_GRAPHS", "0")
    eager = engine()
    assert not eager.runner.enable_graphs
    assert generate(eager, prompt, 16) == grouped
    assert counter.calls > calls
