"""int4 (W4A16) kernels on the GPU: int4_dequant and the fused dequant-GEMM
against Int4Weight.dequant() and an fp64 oracle (bound derived in
int4_util.bound, self-checked on CPU in test_int4.py), the large-M route,
determinism under graph replay, and the engine end to end."""
import pytest
import torch
import torch.nn.functional as F

from int4_util import (
    assert_within_bound, generate, random_awq, write_awq_checkpoint,
)
from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_int4 import Int4Linear, Int4Weight

pytestmark = pytest.mark.gpu

DEV = "cuda"


def weight(N, K, g, seed=0):
    return Int4Weight.from_codes(*random_awq(N, K, g, seed=seed)[3])


# ------------------------------------------------------------ 1. dequant
@pytest.mark.parametrize("g", [32, 64, 128])
@pytest.mark.parametrize("N,K", [(16, 128), (48, 384)])
def test_dequant_bit_equal(N, K, g):
    w = weight(N, K, g, seed=N + g)
    got = ops.int4_dequant(w.to(DEV))
    assert got.dtype == torch.bfloat16 and got.shape == (N, K)
    assert torch.equal(got.cpu(), w.dequant())
    # ragged last chunk (K % 128 = 32) and an out= buffer with a guard row
    w = weight(16, 160, 32, seed=5)
    buf = torch.full((17, 160), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.int4_dequant(w.to(DEV), out=buf[:16])
    assert torch.equal(buf[:16].cpu(), w.dequant())
    assert bool((buf[16] == 7.0).all())


# ------------------------------------------------------------- 2. needle
@pytest.mark.parametrize("g", [32, 128])
def test_needle_every_k(g):
    """x = 64 one-hot rows at k0 + r: y[r, n] is w[n, k0 + r] exactly (one
    nonzero product), for every k of K = 384 (3 chunks of 128 over an 8-wave
    K-split, group boundaries included)."""
    N, K = 48, 384
    w = weight(N, K, g, seed=3)
    ref = w.dequant()
    wd = w.to(DEV)
    for k0 in range(0, K, 64):
        x = torch.zeros(64, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(64), k0 + torch.arange(64)] = 1.0
        y = ops.int4_linear(x, wd)
        assert torch.equal(y.cpu(), ref[:, k0 : k0 + 64].t()), k0


# ----------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("scale", [2.0**-14, 1.0, 2.0**7])
def test_extreme_codes(scale):
    N, K, g = 16, 512, 128
    G = K // g
    s = torch.full((N, G), scale).half()
    lo = (torch.zeros(N, K, dtype=torch.uint8),
          torch.full((N, G), 15, dtype=torch.uint8))       # q - z = -15
    hi = (torch.full((N, K), 15, dtype=torch.uint8),
          torch.zeros(N, G, dtype=torch.uint8))            # q - z = +15
    gsel = (torch.arange(G) % 2).bool()                    # adjacent groups
    checker = (
        torch.where(gsel.repeat_interleave(g), hi[0], lo[0]),
        torch.where(gsel, hi[1], lo[1]),
    )
    torch.manual_seed(0)
    x = torch.randn(17, K).to(torch.bfloat16).to(DEV)
    for q, z in (lo, hi, checker):
        w = Int4Weight.from_codes(q, z, s)
        wd = w.to(DEV)
        assert torch.equal(ops.int4_dequant(wd).cpu(), w.dequant())
        assert_within_bound(ops.int4_linear(x, wd), x, w.dequant(),
                            what=f"extreme s={scale}")


# ----------------------------------------------------------- 4. numerics
@pytest.fixture(scope="module")
def numerics_weights():
    return {g: weight(48, 512, g, seed=20 + g) for g in (32, 64, 128)}


@pytest.mark.parametrize("g", [32, 64, 128])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33, 64])
def test_fused_numerics(numerics_weights, M, g):
    w = numerics_weights[g]
    torch.manual_seed(M)
    x = torch.randn(M, 512).to(torch.bfloat16).to(DEV)
    y = ops.int4_linear(x, w.to(DEV))
    assert y.shape == (M, 48) and y.dtype == torch.bfloat16
    assert_within_bound(y, x, w.dequant(), what=f"M={M} g={g}")


def test_fused_row_strided_x(numerics_weights):
    w = numerics_weights[64]
    torch.manual_seed(1)
    big = torch.randn(33, 3 * 512).to(torch.bfloat16).to(DEV)
    x = big[:, 512:1024]  # row stride 1536, contiguous last dim
    assert not x.is_contiguous()
    y = ops.int4_linear(x, w.to(DEV))
    assert_within_bound(y, x, w.dequant(), what="strided x")
    assert torch.equal(y, ops.int4_linear(x.contiguous(), w.to(DEV)))


def test_fused_plan():
    """Column tiles per workgroup: the widest of 4, 2, 1 that divides N / 16
    and leaves 160 workgroups (256 up to M = 16); 1 at M = 1; no 4 above
    M = 48."""
    from kubeai_amd import _C

    for N, M, want in [
        (5088, 48, 1), (5120, 48, 2), (10208, 48, 2), (10240, 48, 4),
        (10240, 17, 4), (10240, 16, 2), (8176, 16, 1), (8192, 16, 2),
        (16384, 16, 4), (16384, 64, 2), (16384, 1, 1), (48, 64, 1),
    ]:
        assert _C.int4_gemm_tiles(N, M) == want, (N, M)


@pytest.mark.parametrize("N,tiles", [(5120, 2), (10240, 4)])
def test_fused_wide_workgroups(N, tiles):
    """The smallest N at which a workgroup of the fused kernel owns 2 and 4
    column tiles: every k by needle, then the bound on a ragged M."""
    from kubeai_amd import _C

    K, g, R = 384, 64, 48
    assert _C.int4_gemm_tiles(N, R) == tiles
    gen = torch.Generator().manual_seed(N)
    w = Int4Weight.from_codes(
        torch.randint(0, 16, (N, K), generator=gen, dtype=torch.uint8),
        torch.randint(0, 16, (N, K // g), generator=gen, dtype=torch.uint8),
        (torch.rand(N, K // g, generator=gen) * 0.02 + 0.001).half(),
    )
    ref = w.dequant()
    wd = w.to(DEV)
    for k0 in range(0, K, R):
        x = torch.zeros(R, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(R), k0 + torch.arange(R)] = 1.0
        assert torch.equal(ops.int4_linear(x, wd).cpu(), ref[:, k0 : k0 + R].t())
    torch.manual_seed(N)
    x = torch.randn(17, K).to(torch.bfloat16).to(DEV)
    assert_within_bound(ops.int4_linear(x, wd), x, ref, what=f"N={N}")
    assert_within_bound(ops.int4_linear(x[:1], wd), x[:1], ref, what=f"N={N} M=1")


# ------------------------------------------------------ 5. large-M route
@pytest.mark.parametrize("M", [65, 200])
def test_large_m_route(numerics_weights, M):
    """M > 64 runs int4_dequant + F.linear. The library GEMM accumulates in
    fp32 and rounds once to bf16, which is what the bound already allows,
    so its rounding term is not widened: out_ulp stays 2^-9."""
    w = numerics_weights[128]
    torch.manual_seed(M)
    x = torch.randn(M, 512).to(torch.bfloat16).to(DEV)
    y = ops.int4_linear(x, w.to(DEV))
    assert y.shape == (M, 48)
    assert_within_bound(y, x, w.dequant(), what=f"large M={M}")


# ------------------------------------------------------- 6. determinism
def test_deterministic_and_graph_replay(numerics_weights):
    wd = numerics_weights[64].to(DEV)
    torch.manual_seed(2)
    x = torch.randn(33, 512).to(torch.bfloat16).to(DEV)
    eager = ops.int4_linear(x, wd)
    assert torch.equal(eager, ops.int4_linear(x, wd))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.int4_linear(x, wd)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


# ------------------------------------------------------------ 7. engine
def test_engine_int4_graphs_and_eager(tmp_path, monkeypatch):
    def engine(model, device, **kw):
        return LLMEngine(
            EngineConfig(model=model, device=device, num_gpu_blocks=128,
                         max_model_len=512, seed=3, **kw)
        )

    src = engine("llama-tiny", "cpu")
    ckpt = write_awq_checkpoint(src.runner.model, tmp_path / "awq", group=64)
    prompt = list(range(10, 60))

    eng = engine(ckpt, DEV, quantization="int4")
    assert eng.runner.enable_graphs
    with_graphs = generate(eng, prompt, 16)
    assert len(with_graphs) == 16
    assert eng.runner._graphs, "decode did not go through a captured graph"

    layer = eng.runner.model.layers[0]
    lin = layer.self_attn.qkv_proj
    assert isinstance(lin, Int4Linear) and lin.qweight.is_cuda
    torch.manual_seed(4)
    x = torch.randn(8, lin.in_features).to(torch.bfloat16).to(DEV)
    assert_within_bound(lin(x), x, lin.weight, what="engine qkv_proj")

    monkeypatch.setenv("KUBEAI_GRAPHS", "0")
    eager = engine(ckpt, DEV, quantization="int4")
    assert not eager.runner.enable_graphs
    assert generate(eager, prompt, 16) == with_graphs
