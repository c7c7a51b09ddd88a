"""MXFP4 (W4A8) kernels on the GPU: the scaled-MFMA GEMM against exact data
and an fp64 oracle, row independence, mxfp4_dequant, the module and layer
dispatch, host errors, and the engine end to end."""
import types

import pytest
import torch
import torch.nn.functional as F

from int4_util import generate
from kubeai_amd import _C, ops
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_mxfp4 import Mxfp4Linear, Mxfp4Weight
from kubeai_amd.engine.runner import ModelRunner
from kubeai_amd.models.config import PRESETS
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
# fewer chunks than waves; a partial last chunk; every wave takes at least two
# chunks (18 chunks over 8 waves) with a partial last one; and the steady
# state: 66 chunks, so waves take 8 or 9 steps (every register-ring depth
# refills a slot that is then read), two scale words per lane, a partial last
# chunk, and an N at which a workgroup can own 1, 2 or 4 column tiles
SHAPES = [(48, 384), (16, 160), (32, 2208), (64, 8352)]
MS = [1, 5, 17, 33, 64]
E4M3 = torch.float8_e4m3fn


def gemm(xq, xs, w, n_tiles=0):
    y = torch.empty((xq.shape[0], w.N), dtype=torch.bfloat16, device=DEV)
    _C.mxfp4_gemm(y, xq, xs, w.qp, w.sp, w.N, w.K, n_tiles)
    return y


@pytest.fixture(scope="module")
def exact():
    """Per shape: a weight over all 16 codes with block exponents 126..129,
    64 rows of integers in [-8, 8] and power-of-two row scales, and the fp64
    product. Every product is a multiple of 0.5 * 2^-1 = 2^-2 of magnitude at
    most 8 * 6 * 2^2 = 192, so a sum of K <= 8352 of them is, in units of
    2^-2, an integer below 8352 * 768 < 2^23: every partial sum is exact in
    fp32 in any order, and xs is a power of two, so bf16 is the one rounding."""
    out = {}
    for N, K in SHAPES:
        gen = torch.Generator().manual_seed(N * K)
        codes = torch.randint(0, 256, (N, K // 2), generator=gen, dtype=torch.uint8)
        scales = torch.randint(126, 130, (N, K // 32), generator=gen, dtype=torch.uint8)
        w = Mxfp4Weight.from_codes(codes, scales)
        x = torch.randint(-8, 9, (64, K), generator=gen).float()
        xs = torch.pow(2.0, torch.randint(-3, 3, (64,), generator=gen).float())
        acc = x.double() @ w.dequant().double().t()
        out[N, K] = (w.to(DEV), x.to(E4M3).to(DEV), xs.to(DEV), acc)
    return out


@pytest.fixture(scope="module")
def random():
    """Per shape: a round-to-nearest weight, quant_fp8 rows of a normal x, and
    the fp64 oracle over the very bytes the kernel receives."""
    out = {}
    for N, K in SHAPES:
        torch.manual_seed(N + K)
        w = Mxfp4Weight.quantize_rtn(torch.randn(N, K) * 0.05)
        xq, xs = ref.quant_fp8((torch.randn(64, K) * 3).to(torch.bfloat16))
        xd, wd = xq.double(), w.dequant().double()
        out[N, K] = (w.to(DEV), xq.to(DEV), xs.to(DEV).float(),
                     xd @ wd.t(), xd.abs() @ wd.abs().t())
    return out


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_exact_data(exact, N, K, M):
    w, xq, xs, acc = exact[N, K]
    assert _C.mxfp4_plan(M, N) == ((M + 15) // 16, 1)
    y = ops.mxfp4_linear(xq[:M], xs[:M], w)
    want = (acc[:M] * xs[:M].cpu().double().view(-1, 1)).to(torch.bfloat16)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_random_against_fp64(random, N, K, M):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 A + 1e-30: one bf16 rounding, doubled,
    plus the worst case of any-order fp32 summation of K exact terms, doubled
    (the matrix unit's adds are not documented as round-to-nearest).
    Worst err / bound measured on an MI355X: see profiles/r14_mxfp4.md."""
    w, xq, xs, acc, mag = random[N, K]
    assert _C.mxfp4_plan(M, N) == ((M + 15) // 16, 1)
    y = ops.mxfp4_linear(xq[:M], xs[:M].view(-1, 1), w).cpu().double()
    s = xs[:M].cpu().double().view(-1, 1)
    want = acc[:M] * s
    bound = 2.0**-8 * want.abs() + K * 2.0**-23 * (mag[:M] * s) + 1e-30
    ratio = ((y - want).abs() / bound).max().item()
    print(f"mxfp4 N={N} K={K} M={M}: worst err/bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("N,K", SHAPES)
def test_row_independence(N, K):
    torch.manual_seed(K)
    w = Mxfp4Weight.quantize_rtn(torch.randn(N, K)).to(DEV)
    xq, xs = ops.quant_fp8(torch.randn(64, K).to(torch.bfloat16).to(DEV))
    batch = gemm(xq, xs, w, 1)
    for nt in (1, 2, 4):
        if (N // 16) % nt == 0:
            assert torch.equal(gemm(xq, xs, w, nt), batch), nt
            for r in (0, 5, 16, 31, 47, 63):
                alone = gemm(xq[r : r + 1], xs[r : r + 1], w, nt)
                assert torch.equal(alone[0], batch[r]), (nt, r)


@pytest.mark.parametrize("N,K", SHAPES)
def test_dequant_and_large_m_route(exact, N, K):
    w = exact[N, K][0]
    deq = w.to("cpu").dequant()
    buf = torch.full((N + 1, K), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.mxfp4_dequant(w, out=buf[:N])
    assert torch.equal(buf[:N].cpu(), deq) and bool((buf[N] == 7.0).all())
    torch.manual_seed(N)
    x = torch.randn(65, K).to(torch.bfloat16).to(DEV)
    assert torch.equal(Mxfp4Linear(w)(x), F.linear(x, deq.to(DEV)))


def test_module_dispatch(random):
    w = random[48, 384][0]
    bias = torch.nn.Parameter(torch.randn(48).to(torch.bfloat16).to(DEV))
    lin = Mxfp4Linear(w, bias)
    torch.manual_seed(0)
    x = torch.randn(33, 384).to(torch.bfloat16).to(DEV)
    xq, xs = ops.quant_fp8(x)
    assert torch.equal(lin(x), lin.forward_quantized(xq, xs))
    assert torch.equal(lin(x), ops.mxfp4_linear(xq, xs, w) + bias)
    assert torch.equal(lin.weight.cpu(), w.to("cpu").dequant())


def test_host_errors(random):
    """Each raises before any launch: the pointers are valid and the device
    is still healthy afterwards."""
    w, xq, xs = random[16, 160][:3]
    lin = Mxfp4Linear(w)
    wide = torch.zeros((8, 208), dtype=torch.uint8, device=DEV).view(E4M3)
    xq65 = xq.view(torch.uint8).repeat(2, 1)[:65].view(E4M3)
    bad = [
        lambda: gemm(xq[:0], xs[:0], w),                      # M = 0
        lambda: lin.forward_quantized(xq65, xs.repeat(2)[:65]),  # M = 65
        lambda: gemm(wide[:, 1:161], xs[:8], w),              # misaligned rows
        lambda: gemm(xq[:8], xs[:9], w),                      # xs shape
        lambda: gemm(xq[:8], xs[:16].view(8, 2), w),
        lambda: gemm(wide[:, :192], xs[:8], w),               # K mismatch
        lambda: gemm(xq[:8].cpu(), xs[:8], w),                # one device
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert gemm(xq[:8], xs[:8], w).shape == (8, 16)


def engine(model="llama-tiny", **kw):
    return LLMEngine(EngineConfig(
        model=model, device=DEV, num_gpu_blocks=128, max_model_len=512,
        seed=3, quantization="mxfp4", **kw,
    ))


def test_engine_layers_graphs_and_determinism(monkeypatch):
    eng = engine()
    assert eng.runner.enable_graphs
    layer = eng.runner.model.layers[0]
    assert isinstance(layer.self_attn.qkv_proj, Mxfp4Linear)
    assert layer.self_attn.qkv_proj.qweight.is_cuda

    def fb(T):
        return types.SimpleNamespace(
            input_ids=torch.zeros(T, dtype=torch.int32), lora_ids=None
        )

    assert layer.fp8_fused(fb(40), True) and layer.fp8_fused(fb(64), True)
    assert not layer.fp8_fused(fb(65), True)
    assert not layer.fp8_fused(fb(40), False)

    # a 40-token prefill takes the fused branch, a 65-token one the bf16
    # branch and the dequant route; decode steps replay a captured graph
    prompts = [list(range(10, 50)), list(range(100, 165)), [7, 8, 9]]
    with_graphs = [generate(eng, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)]
    assert eng.runner._graphs, "decode did not go through a captured graph"
    again = engine()
    assert [generate(again, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)] \
        == with_graphs
    monkeypatch.setenv("KUBEAI_GRAPHS", "0")
    eager = engine()
    assert not eager.runner.enable_graphs
    assert [generate(eager, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)] \
        == with_graphs


def test_moe_and_tp_are_rejected():
    with pytest.raises(NotImplementedError):
        engine("mixtral-tiny")
    with pytest.raises(NotImplementedError):
        ModelRunner(PRESETS["llama-tiny"], device=DEV, num_gpu_blocks=16,
                    quantization="mxfp4", tp_group=object())
