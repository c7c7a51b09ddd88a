"""Grouped fp8 MoE experts on the GPU: fp8_moe_gemm's operand map with exact
integer data, random data against an fp64 oracle with a derived bound, row
independence, skewed and invalid routings, an unrouted expert that must not be
read, the whole block against its parts and against MoEMLP's dense expert
loop, module dispatch, graph replay under a changed routing, host errors and
the engine end to end."""
import dataclasses

import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams
from kubeai_amd.engine.quant import Fp8ExpertGroup, Fp8Linear, convert_to_fp8
from kubeai_amd.models.config import PRESETS
from kubeai_amd.models.llama import MoEMLP
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
E, TOPK = 4, 2
FP8 = torch.float8_e4m3fn
# chunks of 128 over the 8-wave K split: 3 chunks (fewer than waves); 2 chunks
# with a partial last one; 18 chunks (every wave takes at least two) with a
# partial last one
SHAPES = [(48, 384), (16, 160), (32, 2208)]
TS = [1, 5, 17, 33, 64]
SENTINEL = 7.0


def bits(t):
    return t.contiguous().view(torch.int16)


def random_routing(T, n_experts, k, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.randperm(n_experts, generator=gen)[:k] for _ in range(T)]
    return torch.stack(rows).to(torch.int64)


def linear_from(wq, ws):
    """An Fp8Linear holding exactly these e4m3 [N, K] bytes and fp32 scales."""
    N, K = wq.shape
    lin = Fp8Linear(torch.zeros(N, K, dtype=torch.bfloat16))
    lin.weight_fp8 = wq.to(FP8).contiguous()
    lin.weight_scale = ws.float().reshape(1, N).contiguous()
    return lin


class Experts:
    """E Fp8Linears of one shape: CPU tensors for the oracle, GPU modules and
    their group for the kernel."""

    def __init__(self, linears):
        self.wq = [lin.weight_fp8.clone() for lin in linears]
        self.ws = [lin.weight_scale.reshape(-1).clone() for lin in linears]
        self.dev = [lin.to(DEV) for lin in linears]
        self.group = Fp8ExpertGroup(self.dev)


def integer_experts(N, K, seed):
    """Weights in [-8, 8] (exact in e4m3), scales powers of two."""
    gen = torch.Generator().manual_seed(seed)
    return Experts([
        linear_from(
            torch.randint(-8, 9, (N, K), generator=gen).float(),
            2.0 ** torch.randint(-4, 4, (N,), generator=gen).float(),
        )
        for _ in range(E)
    ])


def random_experts(N, K, seed, n_experts=E):
    torch.manual_seed(seed)
    return Experts([
        Fp8Linear((torch.randn(N, K) * 0.05).to(torch.bfloat16))
        for _ in range(n_experts)
    ])


@pytest.fixture(scope="module")
def int_experts():
    return {s: integer_experts(*s, seed=s[1]) for s in SHAPES}


@pytest.fixture(scope="module")
def rnd_experts():
    return {s: random_experts(*s, seed=s[1]) for s in SHAPES}


def integer_rows(R, K, seed):
    """(xq e4m3 [R, K] of integers in [-8, 8], xs [R] powers of two), CPU."""
    gen = torch.Generator().manual_seed(seed)
    xq = torch.randint(-8, 9, (R, K), generator=gen).float().to(FP8)
    xs = 2.0 ** torch.randint(-4, 4, (R,), generator=gen).float()
    return xq, xs


def random_rows(R, K, seed):
    torch.manual_seed(seed)
    scale = 10.0 ** (torch.rand(R, 1) * 3.0 - 2.0)  # rows of 1e-2 .. 1e1
    return ref.quant_fp8((torch.randn(R, K) * scale).to(torch.bfloat16))


def assert_plan(N, T, n_experts=E, k=TOPK, nt=1):
    from kubeai_amd import _C

    assert _C.fp8_moe_plan(N, T, n_experts, k) == ((T + 15) // 16, nt)


def oracle(xq, xs, selected, experts, row_div):
    """fp64 over the very bytes and scales the kernel receives, CPU tensors:
    (y^ = (sum xq wq) xs ws, A = (sum |xq| |wq|) xs ws) per pair, [T*k, N]."""
    flat = selected.reshape(-1).cpu()
    rows = torch.arange(flat.numel()) // row_div
    x = xq.cpu().float().double()
    s = xs.cpu().double().reshape(-1, 1)
    yh, A = [], []
    for wq, ws in zip(experts.wq, experts.ws):
        w = wq.float().double()
        yh.append((x @ w.t()) * s * ws.double())
        A.append((x.abs() @ w.abs().t()) * s * ws.double())
    ok = (flat >= 0) & (flat < len(experts.wq))
    e = torch.where(ok, flat, torch.zeros_like(flat))
    return torch.stack(yh)[e, rows], torch.stack(A)[e, rows], ok


def bound_ratio(y, yh, A, K):
    """max of |y - y^| / (2^-7 |y^| + 2 (K + 2) 2^-24 A): the bf16 rounding is
    at most 2^-8 relative, the fp32 sum of K exact products in any order at
    most (K - 1) 2^-24 A, the two scale multiplications add 2 * 2^-24; that
    sum, doubled."""
    lim = 2.0**-7 * yh.abs() + 2.0 * (K + 2) * 2.0**-24 * A
    err = (y.cpu().double() - yh).abs()
    return (err / lim.clamp_min(1e-300)).max().item()


def run(experts, xq, xs, selected, row_div, out=None):
    return ops.fp8_moe_linear(
        xq.to(DEV), xs.to(DEV), selected.to(DEV), experts.group, row_div, out=out
    )


# ------------------------------------- 1. exact integer data, bit for bit
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_data_bit_exact(int_experts, shape, T):
    """Every partial sum is an integer below 2^24 and the scales are powers
    of two, so any summation order gives the same fp32: y is the bf16 rounding
    of the integer result. A k-slot that A and B do not share shows here."""
    N, K = shape
    experts = int_experts[shape]
    assert_plan(N, T)
    assert 8 * 8 * K < 2**24
    selected = random_routing(T, E, TOPK, seed=T + K)
    for row_div in (TOPK, 1):
        xq, xs = integer_rows(T * TOPK // row_div, K, seed=T + row_div)
        yh, _, ok = oracle(xq, xs, selected, experts, row_div)
        assert bool(ok.all())
        assert torch.equal(yh.float().double(), yh), "the result is exact in fp32"
        want = yh.float().to(torch.bfloat16)
        y = run(experts, xq, xs, selected, row_div)
        assert y.shape == (T * TOPK, N) and y.dtype == torch.bfloat16
        assert torch.equal(bits(y.cpu()), bits(want)), row_div


# ----------------------------------- 2. random data against an fp64 oracle
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_data_within_bound(rnd_experts, shape, T):
    N, K = shape
    experts = rnd_experts[shape]
    assert_plan(N, T)
    selected = random_routing(T, E, TOPK, seed=3 * T + K)
    worst = 0.0
    for row_div in (TOPK, 1):
        xq, xs = random_rows(T * TOPK // row_div, K, seed=T + row_div)
        yh, A, _ = oracle(xq, xs, selected, experts, row_div)
        y = run(experts, xq, xs, selected, row_div)
        worst = max(worst, bound_ratio(y, yh, A, K))
    print(f"fp8_moe_gemm N={N} K={K} T={T}: max err/bound = {worst:.4f}")
    assert worst <= 1.0


# ------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("shape", SHAPES)
def test_row_is_independent_of_the_batch(rnd_experts, shape):
    """The row of pair p at T = 33 is, as bits, the T = 1 call with that
    token alone."""
    N, K = shape
    experts = rnd_experts[shape]
    T = 33
    selected = random_routing(T, E, TOPK, seed=K).to(DEV)
    xq, xs = (t.to(DEV) for t in random_rows(T, K, seed=K))
    y = run(experts, xq, xs, selected, TOPK)
    for t in range(T):
        alone = run(experts, xq[t : t + 1], xs[t : t + 1], selected[t : t + 1], TOPK)
        assert torch.equal(bits(alone), bits(y[t * TOPK : (t + 1) * TOPK])), t


def test_row_is_independent_of_the_tiles():
    """Workgroups of 1, 2 and 4 column tiles at every row-tile count, asked
    for through n_tiles (N = 64 is four tiles; the plan itself takes 1)."""
    from kubeai_amd import _C

    N, K = 64, 2208
    experts = random_experts(N, K, seed=64)
    table = experts.group.table
    for T in (5, 17, 33, 64):
        assert_plan(N, T)
        selected = random_routing(T, E, TOPK, seed=T).to(DEV)
        xq, xs = (t.to(DEV) for t in random_rows(T, K, seed=T))
        got = {}
        for nt in (1, 2, 4):
            if T > 48 and nt == 4:
                continue
            y = torch.full((T * TOPK, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
            _C.fp8_moe_gemm(y, xq, xs, selected, table, TOPK, E, N, K, nt)
            got[nt] = y
        yh, A, _ = oracle(xq, xs, selected, experts, TOPK)
        assert bound_ratio(got[1], yh, A, K) <= 1.0
        for nt, y in got.items():
            assert torch.equal(bits(y), bits(got[1])), (T, nt)
        # T = 5 rows at T = 64's four row tiles: the same tokens, the same bits
        if T == 5:
            first = got[1]
        if T == 64:
            sel5 = random_routing(5, E, TOPK, seed=5).to(DEV)
            selected[:5] = sel5
            xq5, xs5 = (t.to(DEV) for t in random_rows(5, K, seed=5))
            xq.view(torch.uint8)[:5] = xq5.view(torch.uint8)
            xs[:5] = xs5
            y = run(experts, xq, xs, selected, TOPK)
            assert torch.equal(bits(y[: 5 * TOPK]), bits(first))
    y = torch.empty(64 * TOPK, N, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="4 x 4"):
        _C.fp8_moe_gemm(y, xq, xs, selected, table, TOPK, E, N, K, 4)


def test_wide_workgroups_planned():
    """The smallest N (a multiple of 64) at which the plan itself takes 4
    column tiles for E = 4, k = 2, T = 17 (just under 4 experts expected x
    101 column blocks reach the floor of 400 workgroups, x 100 do not), on
    exact integer data."""
    N, K, T = 6464, 160, 17
    assert_plan(N, T, nt=4)
    assert_plan(N - 64, T, nt=2)
    experts = integer_experts(N, K, seed=1)
    selected = random_routing(T, E, TOPK, seed=3)
    xq, xs = integer_rows(T, K, seed=2)
    yh, _, _ = oracle(xq, xs, selected, experts, TOPK)
    y = run(experts, xq, xs, selected, TOPK)
    assert torch.equal(bits(y.cpu()), bits(yh.float().to(torch.bfloat16)))


# ---------------------------------------------------------------- 4. routing
def skewed(second):
    """T = 64, every token's first choice expert 2, second choices given as
    (expert, count) runs."""
    col = torch.cat([torch.full((n,), e) for e, n in second])
    assert col.numel() == 64
    return torch.stack([torch.full((64,), 2), col], dim=1).to(torch.int64)


@pytest.mark.parametrize("second", [
    # expert 2 takes 64 pairs (all four row tiles); expert 0 takes 17, on
    # the far side of a tile boundary, expert 1 takes 1
    [(0, 17), (1, 1), (3, 46)],
    # expert 3 takes none; 16 pairs fill one tile exactly
    [(0, 16), (1, 48)],
])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_skewed_routing(int_experts, shape, second):
    N, K = shape
    experts = int_experts[shape]
    T = 64
    assert_plan(N, T)
    selected = skewed(second)
    xq, xs = integer_rows(T, K, seed=K)
    yh, _, _ = oracle(xq, xs, selected, experts, TOPK)
    buf = torch.full((T * TOPK + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = run(experts, xq, xs, selected, TOPK, out=buf[: T * TOPK])
    assert y.data_ptr() == buf.data_ptr()
    assert torch.equal(bits(y.cpu()), bits(yh.float().to(torch.bfloat16)))
    assert bool((buf[T * TOPK] == SENTINEL).all())


def test_any_routing_stays_in_bounds(int_experts):
    """Ids outside [0, E) belong to no workgroup: their rows are not written,
    the others are right. A token that names one expert twice (invalid: its
    results are unspecified) still writes nothing outside y."""
    shape = SHAPES[0]
    N, K = shape
    experts = int_experts[shape]
    T = 64
    selected = random_routing(T, E, TOPK, seed=9)
    selected[3, 0], selected[10, 1], selected[40, 0] = -1, E, 2**40 + 1
    xq, xs = integer_rows(T, K, seed=9)
    yh, _, ok = oracle(xq, xs, selected, experts, TOPK)
    assert int((~ok).sum()) == 3
    want = yh.float().to(torch.bfloat16)
    want[~ok] = SENTINEL
    buf = torch.full((T * TOPK + 1, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = run(experts, xq, xs, selected, TOPK, out=buf[: T * TOPK])
    assert torch.equal(bits(y.cpu()), bits(want))
    assert bool((buf[T * TOPK] == SENTINEL).all())

    twice = torch.zeros(T, TOPK, dtype=torch.int64)  # 128 pairs > 64 rows
    buf.fill_(SENTINEL)
    run(experts, xq, xs, twice, TOPK, out=buf[: T * TOPK])
    torch.cuda.synchronize()
    assert bool((buf[T * TOPK] == SENTINEL).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_needle(rnd_experts, shape):
    """xq[t] is 1 at k = t with scale 1, so y[t*k + j, n] is
    wq_e[n, t] * ws_e[n] exactly for e = selected[t, j]: a wrong row gather,
    expert pointer or pair index shows as a wrong weight."""
    N, K = shape
    experts = rnd_experts[shape]
    T = 33
    selected = random_routing(T, E, TOPK, seed=K)
    x = torch.zeros(T, K)
    x[torch.arange(T), torch.arange(T)] = 1.0
    y = run(experts, x.to(FP8), torch.ones(T), selected, TOPK).cpu()
    for t in range(T):
        for j in range(TOPK):
            e = int(selected[t, j])
            want = (experts.wq[e][:, t].float() * experts.ws[e]).to(torch.bfloat16)
            assert torch.equal(bits(y[t * TOPK + j]), bits(want)), (t, j)


def test_row_strided_x(rnd_experts):
    shape = SHAPES[2]
    N, K = shape
    experts = rnd_experts[shape]
    T = 17
    selected = random_routing(T, E, TOPK, seed=1).to(DEV)
    big, xs = random_rows(T, 3 * K, seed=1)
    xq = big.to(DEV)[:, K : 2 * K]
    assert not xq.is_contiguous()
    xs = xs.to(DEV)
    y = run(experts, xq, xs, selected, TOPK)
    assert torch.equal(bits(y), bits(run(experts, xq.contiguous(), xs, selected, TOPK)))
    yh, A, _ = oracle(xq, xs, selected, experts, TOPK)
    assert bound_ratio(y, yh, A, K) <= 1.0


# ---------------------------------------------------------------- the block
def make_block(n_experts, k, H, inter, seed, fp8=True):
    cfg = dataclasses.replace(
        PRESETS["mixtral-tiny"], num_local_experts=n_experts,
        num_experts_per_tok=k, hidden_size=H, intermediate_size=inter,
    )
    torch.manual_seed(seed)
    mlp = MoEMLP(cfg).to(torch.bfloat16)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    if fp8:
        convert_to_fp8(mlp)
    return mlp.to(DEV)


def route(mlp, x):
    router = torch.nn.functional.linear(x.float(), mlp.gate.weight.float())
    weights, selected = torch.topk(router, mlp.top_k, dim=-1)
    return selected, torch.softmax(weights, dim=-1).to(x.dtype)


def experts_of(mlp, name):
    """The oracle's view (CPU bytes and scales) of a block's projection."""
    view = Experts.__new__(Experts)
    view.wq = [getattr(ex, name).weight_fp8.cpu() for ex in mlp.experts]
    view.ws = [getattr(ex, name).weight_scale.reshape(-1).cpu() for ex in mlp.experts]
    return view


@pytest.fixture(scope="module")
def block_e8():
    return make_block(8, 2, 512, 512, seed=1)


# ------------------------------------ 5. an unrouted expert is not read
def test_unrouted_expert_is_not_read():
    mlp = make_block(4, 2, 256, 512, seed=0)
    gu, dn = mlp.fp8_groups()
    T = 17
    torch.manual_seed(T)
    x = torch.randn(T, 256).to(torch.bfloat16).to(DEV)
    selected = random_routing(T, 3, 2, seed=4).to(DEV)  # experts 0, 1, 2 only
    weights = torch.softmax(torch.randn(T, 2), dim=-1).to(torch.bfloat16).to(DEV)
    ordinary = ops.fp8_moe_mlp(x, selected, weights, gu, dn)
    for lin in (mlp.experts[3].gate_up_proj, mlp.experts[3].down_proj):
        lin.weight_fp8.view(torch.uint8).fill_(0x7F)  # e4m3fn NaN
        lin.weight_scale.fill_(float("nan"))
    assert bool(mlp.experts[3].down_proj.weight_fp8.float().isnan().all())
    assert mlp.fp8_groups()[0] is gu, "filled in place: the table stands"
    poisoned = ops.fp8_moe_mlp(x, selected, weights, gu, dn)
    assert bool(torch.isfinite(poisoned).all())
    assert torch.equal(bits(poisoned), bits(ordinary))


# ------------------------------------------------------------------ 6. block
@pytest.mark.parametrize("T", [1, 17, 64])
def test_block_is_its_four_ops(block_e8, T):
    mlp = block_e8
    gu, dn = mlp.fp8_groups()
    assert gu.table.is_cuda and gu.table.tolist() == [
        [ex.gate_up_proj.weight_fp8.data_ptr(),
         ex.gate_up_proj.weight_scale.data_ptr()] for ex in mlp.experts
    ]
    assert_plan(gu.N, T, n_experts=8)
    assert_plan(dn.N, T, n_experts=8)
    torch.manual_seed(T)
    x = torch.randn(T, 512).to(torch.bfloat16).to(DEV)
    selected, weights = route(mlp, x)
    got = ops.fp8_moe_mlp(x, selected, weights, gu, dn)
    assert got.shape == x.shape and got.dtype == x.dtype

    xq, xs = ops.quant_fp8(x)
    h = ops.fp8_moe_linear(xq, xs, selected, gu, 2)
    a8, a_s = ops.silu_and_mul_fp8(h)
    y = ops.fp8_moe_linear(a8, a_s, selected, dn, 1)
    out = ops.moe_combine(y, selected, weights, 8)
    assert torch.equal(bits(got), bits(out))

    yh, A, _ = oracle(xq, xs, selected, experts_of(mlp, "gate_up_proj"), 2)
    r_up = bound_ratio(h, yh, A, gu.K)
    yh, A, _ = oracle(a8, a_s, selected, experts_of(mlp, "down_proj"), 1)
    r_down = bound_ratio(y, yh, A, dn.K)
    print(f"fp8 block T={T}: gate_up err/bound = {r_up:.4f}, down = {r_down:.4f}")
    assert r_up <= 1.0 and r_down <= 1.0
    assert torch.equal(
        out.cpu(), ref.moe_combine(y.cpu(), selected.cpu(), weights.cpu(), 8)
    )


def unquantized_block(mlp, x, selected, weights):
    """The block in fp64 with the dequantized weights and no activation
    quantization, on the CPU."""
    xd = x.cpu().double()
    sel, w = selected.cpu(), weights.cpu().double()
    out = torch.zeros_like(xd)
    for e, ex in enumerate(mlp.experts):
        gu, dn = ex.gate_up_proj, ex.down_proj
        wg = gu.weight_fp8.cpu().double() * gu.weight_scale.cpu().double().reshape(-1, 1)
        wd = dn.weight_fp8.cpu().double() * dn.weight_scale.cpu().double().reshape(-1, 1)
        gate, up = (xd @ wg.t()).chunk(2, dim=-1)
        contrib = (torch.nn.functional.silu(gate) * up) @ wd.t()
        out += contrib * (w * (sel == e)).sum(dim=1, keepdim=True)
    return out


@pytest.mark.parametrize("T", [1, 17, 64])
def test_block_against_dense_loop(block_e8, T, monkeypatch):
    """The grouped block and the dense loop differ from each other by no more
    than the dense loop differs from the unquantized result."""
    mlp = block_e8
    torch.manual_seed(100 + T)
    x = torch.randn(T, 512).to(torch.bfloat16).to(DEV)
    selected, weights = route(mlp, x)
    monkeypatch.delenv("KUBEAI_FP8_MOE_T", raising=False)
    dense = mlp(x)
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    grouped = mlp(x)
    assert torch.equal(
        bits(grouped), bits(ops.fp8_moe_mlp(x, selected, weights, *mlp.fp8_groups()))
    )
    exact = unquantized_block(mlp, x, selected, weights)
    e_dense = ((dense.cpu().double() - exact).norm() / exact.norm()).item()
    d = ((grouped.double() - dense.double()).norm() / dense.double().norm()).item()
    print(f"fp8 block T={T}: e_dense = {e_dense:.3e}, d = {d:.3e}")
    assert d <= e_dense


# -------------------------------------------------------- 7. module dispatch
class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def test_module_dispatch(block_e8, monkeypatch):
    mlp = block_e8
    counter = Counter(ops.fp8_moe_mlp)
    monkeypatch.setattr(ops, "fp8_moe_mlp", counter)
    x = torch.randn(65, 512).to(torch.bfloat16).to(DEV)
    monkeypatch.delenv("KUBEAI_FP8_MOE_T", raising=False)
    mlp(x[:4])
    assert counter.calls == 0, "the default is the dense loop"
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    mlp(x)
    assert counter.calls == 0
    mlp(x[:64])
    assert counter.calls == 1
    mlp(x[:1])
    assert counter.calls == 2
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "16")
    mlp(x[:17])
    assert counter.calls == 2
    mlp(x[:16])
    assert counter.calls == 3
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "0")
    mlp(x[:16])
    assert counter.calls == 3
    # bf16 experts have no fp8 groups
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    plain = make_block(4, 2, 256, 512, seed=2, fp8=False)
    assert plain.fp8_groups() is None
    plain(x[:8, :256].contiguous())
    assert counter.calls == 3


# ------------------------------------------------------------------ 8. graph
def test_routing_is_read_at_replay(block_e8, monkeypatch):
    """The whole module (router, topk, grouped block) captured with one x;
    another x, with another routing, is served by the replay."""
    mlp = block_e8
    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    T = 17
    torch.manual_seed(5)
    cases = []
    for _ in range(2):
        x = torch.randn(T, 512).to(torch.bfloat16).to(DEV)
        cases.append((x, route(mlp, x)[0], mlp(x)))
    assert not torch.equal(cases[0][1], cases[1][1])
    assert not torch.equal(cases[0][2], cases[1][2])
    static_x = cases[0][0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mlp(static_x)
    for x, _, eager in (cases[1], cases[0], cases[1]):
        static_x.copy_(x)
        results = []
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            results.append(out.clone())
        assert torch.equal(bits(results[0]), bits(eager))
        assert torch.equal(bits(results[0]), bits(results[1]))


# ------------------------------------------------------------ 9. host errors
def test_host_errors(int_experts):
    from kubeai_amd import _C

    shape = SHAPES[0]
    N, K = shape
    group = int_experts[shape].group

    def call(xq, selected, row_div, table=group.table, N=N, K=K, nt=0,
             y_rows=None, xs=None):
        n = selected.numel() if y_rows is None else y_rows
        y = torch.full((n, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
        if xs is None:
            xs = torch.ones(xq.shape[0], device=DEV)
        _C.fp8_moe_gemm(y, xq, xs, selected, table, row_div, E, N, K, nt)
        return y

    def xrows(n, K=K):
        return torch.zeros(n, K, device=DEV).to(FP8)

    def sel(T, k):
        return torch.zeros(T, k, dtype=torch.int64, device=DEV)

    call(xrows(4), random_routing(4, E, 2, 0).to(DEV), 2)  # the valid form
    with pytest.raises(RuntimeError, match=r"T in \[1, 64\]"):
        call(xrows(65), sel(65, 2), 2)
    with pytest.raises(RuntimeError, match=r"k in \[1, 8\]"):
        call(xrows(4), sel(4, 9), 9)
    with pytest.raises(RuntimeError, match="N must be a multiple of 16"):
        call(xrows(4), sel(4, 2), 2, N=40)
    with pytest.raises(RuntimeError, match="K must be a multiple of 32"):
        call(xrows(4, 48), sel(4, 2), 2, K=48)
    with pytest.raises(RuntimeError, match=r"table is int64 \[E, 2\]"):
        call(xrows(4), sel(4, 2), 2,
             table=torch.zeros(E, 3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="selected is int64"):
        call(xrows(4), sel(4, 2).to(torch.int32), 2)
    with pytest.raises(RuntimeError, match="rows"):
        call(xrows(4), sel(4, 2), 1)
    with pytest.raises(RuntimeError, match="rows"):
        call(xrows(5), sel(4, 2), 2)
    with pytest.raises(RuntimeError, match="column tiles"):
        call(xrows(4), sel(4, 2), 2, nt=3)
    wide = torch.zeros(4, K + 16, device=DEV).to(FP8)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(wide[:, 1 : K + 1], sel(4, 2), 2)
    with pytest.raises(RuntimeError, match="e4m3fn"):
        call(torch.zeros(4, K, dtype=torch.bfloat16, device=DEV), sel(4, 2), 2)
    with pytest.raises(RuntimeError, match="one scale per row"):
        call(xrows(4), sel(4, 2), 2, xs=torch.ones(3, device=DEV))
    with pytest.raises(RuntimeError, match="y is bf16"):
        call(xrows(4), sel(4, 2), 2, y_rows=7)
    with pytest.raises(RuntimeError, match="table is int64"):
        call(xrows(4), sel(4, 2), 2, table=group.table.cpu())


# --------------------------------------------------------------- 10. engine
def generate_all(eng, prompts, n):
    for i, prompt in enumerate(prompts):
        eng.add_request(
            prompt, SamplingParams(max_tokens=n, ignore_eos=True), request_id=str(i)
        )
    done = {}
    for _ in range(40 * n + 100):
        if not eng.has_work():
            break
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o.output_token_ids
    assert len(done) == len(prompts), "did not finish"
    return [done[str(i)] for i in range(len(prompts))]


def test_engine_grouped_path_tokens(monkeypatch):
    def engine():
        return LLMEngine(
            EngineConfig(model="mixtral-tiny", device=DEV, num_gpu_blocks=128,
                         max_model_len=512, seed=3, quantization="fp8")
        )

    counter = Counter(ops.fp8_moe_mlp)
    monkeypatch.setattr(ops, "fp8_moe_mlp", counter)
    prompts = [list(range(10, 60)), list(range(100, 117)), [7, 8, 9, 10]]

    monkeypatch.setenv("KUBEAI_FP8_MOE_T", "64")
    eng = engine()
    assert eng.runner.enable_graphs
    mlp = eng.runner.model.layers[0].mlp
    assert isinstance(mlp.experts[0].gate_up_proj, Fp8Linear)
    assert mlp.fp8_groups() is not None and mlp.fp8_groups()[0].table.is_cuda
    grouped = generate_all(eng, prompts, 16)
    assert all(len(toks) == 16 for toks in grouped)
    assert eng.runner._graphs, "decode did not go through a captured graph"
    assert counter.calls > 0, "the grouped path did not run"
    del eng

    again = engine()
    assert generate_all(again, prompts, 16) == grouped
    del again

    calls = counter.calls
    monkeypatch.delenv("KUBEAI_FP8_MOE_T")
    dense = engine()
    assert all(len(toks) == 16 for toks in generate_all(dense, prompts, 16))
    assert counter.calls == calls, "unset, the switch still took the grouped path"
