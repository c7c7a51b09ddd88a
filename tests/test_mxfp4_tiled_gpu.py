"""The output-tiled MXFP4 (W4A8) GEMM for steps of more than 64 rows: exact
data and an fp64 oracle in every tile form, row independence, the plan, the
KUBEAI_MXFP4_TILED_M routing, host errors and the engine end to end."""
import types

import pytest
import torch
import torch.nn.functional as F

from int4_util import generate
from kubeai_amd import _C, ops
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_mxfp4 import Mxfp4Linear, Mxfp4Weight
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
E4M3 = torch.float8_e4m3fn
# one column tile inside a BN of 64 / 128 with one full and one partial chunk;
# fewer chunks than one w sweep; 18 chunks, a partial last one, N no multiple
# of BN; 66 chunks (three scale-word groups, the last short and partial) over
# 17 column tiles (a last column block of one tile)
SHAPES = [(16, 160), (48, 384), (160, 2208), (272, 8352)]
# a last row block of one row, full blocks, a last block whose upper row tiles
# are empty, and a ragged last block
MS = [65, 128, 129, 200]
ROWS = 200
FORMS = [(0, 0), (64, 128), (64, 64)]  # (0, 0): the plan's


def tiled(xq, xs, w, form=(0, 0)):
    y = torch.empty((xq.shape[0], w.N), dtype=torch.bfloat16, device=DEV)
    _C.mxfp4_gemm_tiled(y, xq, xs, w.qp, w.sp, w.N, w.K, *form)
    return y


@pytest.fixture(scope="module")
def exact():
    """test_mxfp4_gpu.py's exact construction at 200 rows: all 16 codes, block
    exponents 126..129, integer x in [-8, 8], power-of-two row scales. Every
    product is a multiple of 2^-2 of magnitude at most 192, so a sum of
    K <= 8352 of them is, in units of 2^-2, an integer below 2^23: every
    partial sum is exact in fp32 in any order, whatever M is, and bf16 is the
    one rounding."""
    out = {}
    for N, K in SHAPES:
        gen = torch.Generator().manual_seed(N * K)
        codes = torch.randint(0, 256, (N, K // 2), generator=gen, dtype=torch.uint8)
        scales = torch.randint(126, 130, (N, K // 32), generator=gen, dtype=torch.uint8)
        w = Mxfp4Weight.from_codes(codes, scales)
        x = torch.randint(-8, 9, (ROWS, K), generator=gen).float()
        xs = torch.pow(2.0, torch.randint(-3, 3, (ROWS,), generator=gen).float())
        want = (x.double() @ w.dequant().double().t()) * xs.double().view(-1, 1)
        out[N, K] = (w.to(DEV), x.to(E4M3).to(DEV), xs.to(DEV),
                     want.to(torch.bfloat16))
    return out


@pytest.fixture(scope="module")
def random():
    """Per shape: a round-to-nearest weight, quant_fp8 rows of a normal x, the
    fp64 oracle over the very bytes the kernel receives and its magnitude
    sum, both times the row scale."""
    out = {}
    for N, K in SHAPES:
        torch.manual_seed(N + K)
        w = Mxfp4Weight.quantize_rtn(torch.randn(N, K) * 0.05)
        xq, xs = ref.quant_fp8((torch.randn(ROWS, K) * 3).to(torch.bfloat16))
        xd, wd, s = xq.double(), w.dequant().double(), xs.double().view(-1, 1)
        out[N, K] = (w.to(DEV), xq.to(DEV), xs.to(DEV).float(),
                     (xd @ wd.t()) * s, (xd.abs() @ wd.abs().t()) * s)
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_exact_data(exact, N, K, M, form):
    w, xq, xs, want = exact[N, K]
    assert _C.mxfp4_tiled_plan(M, N) == (64, 64)
    y = tiled(xq[:M], xs[:M], w, form)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    assert torch.equal(y.cpu(), want[:M])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_random_against_fp64(random, N, K, M, form):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 A + 1e-30, the bound of
    test_mxfp4_gpu.py: one bf16 rounding, doubled, plus the worst case of
    any-order fp32 summation of K exact terms, doubled. Worst err / bound
    measured on an MI355X: see profiles/r18_mxfp4_tiled.md."""
    w, xq, xs, want, mag = random[N, K]
    assert _C.mxfp4_tiled_plan(M, N) == (64, 64)
    y = tiled(xq[:M], xs[:M].view(-1, 1), w, form).cpu().double()
    bound = 2.0**-8 * want[:M].abs() + K * 2.0**-23 * mag[:M] + 1e-30
    ratio = ((y - want[:M]).abs() / bound).max().item()
    print(f"mxfp4 tiled N={N} K={K} M={M} form={form}: worst err/bound {ratio:.4f}")
    assert ratio <= 1.0


def test_row_independence(random):
    w, xq, xs = random[272, 8352][:3]
    batch = tiled(xq, xs, w)
    for form in FORMS[1:]:
        assert torch.equal(tiled(xq, xs, w, form), batch), form
        for r in (0, 63, 64, 127, 128, 199):
            alone = tiled(xq[r : r + 1], xs[r : r + 1], w, form)
            assert torch.equal(alone[0], batch[r]), (form, r)


@pytest.mark.parametrize("M,N,want", [
    # 64 x 128 from 448 workgroups of it. 8B o / down, N = 4096, 32 column
    # blocks: 14 row blocks; 8B gate_up, N = 28672, 224 column blocks: 2
    (832, 4096, (64, 64)), (833, 4096, (64, 128)),
    (64, 28672, (64, 64)), (65, 28672, (64, 128)),
    (200, 272, (64, 64)), (1, 16, (64, 64)),
])
def test_plan(M, N, want):
    assert _C.mxfp4_tiled_plan(M, N) == want


def test_routing(random, monkeypatch):
    w, xq = random[48, 384][:2]
    deq = w.to("cpu").dequant().to(DEV)
    bias = torch.nn.Parameter(torch.randn(48).to(torch.bfloat16).to(DEV))
    lin = Mxfp4Linear(w, bias)
    torch.manual_seed(1)
    x = torch.randn(257, 384).to(torch.bfloat16).to(DEV)
    monkeypatch.delenv("KUBEAI_MXFP4_TILED_M", raising=False)
    small = lin(x[:33])
    monkeypatch.setenv("KUBEAI_MXFP4_TILED_M", "256")
    assert ops.mxfp4_m_max() == 256 and ops.MXFP4_M_FUSED == 64
    for M in (65, 200):
        q8, s8 = ops.quant_fp8(x[:M])
        assert torch.equal(lin(x[:M]), tiled(q8, s8, w) + bias), M
        assert torch.equal(lin.forward_quantized(q8, s8), lin(x[:M])), M
    assert torch.equal(lin(x), F.linear(x, deq) + bias)
    with pytest.raises(RuntimeError):
        lin.forward_quantized(*ops.quant_fp8(x))
    assert torch.equal(lin(x[:33]), small)
    monkeypatch.setenv("KUBEAI_MXFP4_TILED_M", "8")
    assert ops.mxfp4_m_max() == 64


def test_host_errors(random):
    """Each raises before any launch: the pointers are valid and the device
    is still healthy afterwards."""
    w, xq, xs = random[16, 160][:3]
    wide = torch.zeros((80, 208), dtype=torch.uint8, device=DEV).view(E4M3)
    bad = [
        lambda: tiled(xq[:0], xs[:0], w),                     # M = 0
        lambda: tiled(wide[:, 1:161], xs[:80], w),            # misaligned rows
        lambda: tiled(xq[:80], xs[:81], w),                   # xs shape
        lambda: tiled(xq[:80], xs[:160].view(80, 2), w),
        lambda: tiled(wide[:, :192], xs[:80], w),             # K mismatch
        lambda: tiled(xq[:80].cpu(), xs[:80], w),             # one device
        lambda: tiled(xq[:80], xs[:80], w, (128, 64)),        # no such form
        lambda: tiled(xq[:80], xs[:80], w, (64, 0)),
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert tiled(xq[:80], xs[:80], w).shape == (80, 16)


def engine(**kw):
    return LLMEngine(EngineConfig(
        model="llama-tiny", device=DEV, num_gpu_blocks=128, max_model_len=512,
        seed=3, quantization="mxfp4", **kw,
    ))


def test_engine_graphs_and_determinism(monkeypatch):
    """100- and 200-token prefills take the fused branch and the tiled kernel.
    Tokens are not compared with a switch-off engine: its bf16 branch has no
    e4m3 activations, the arithmetic differs by design."""
    monkeypatch.setenv("KUBEAI_MXFP4_TILED_M", "256")
    prompts = [list(range(10, 110)), list(range(100, 300)), [7, 8, 9]]
    eng = engine()
    assert eng.runner.enable_graphs
    layer = eng.runner.model.layers[0]

    def fb(T):
        return types.SimpleNamespace(
            input_ids=torch.zeros(T, dtype=torch.int32), lora_ids=None
        )

    assert layer.fp8_fused(fb(65), True) and layer.fp8_fused(fb(256), True)
    assert not layer.fp8_fused(fb(257), True)
    with_graphs = [generate(eng, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)]
    assert eng.runner._graphs, "decode did not go through a captured graph"
    again = engine()
    assert [generate(again, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)] \
        == with_graphs
    chunked = engine(max_num_batched_tokens=32)
    assert all(len(generate(chunked, p, 12, rid=f"r{i}")) == 12
               for i, p in enumerate(prompts))
    monkeypatch.setenv("KUBEAI_GRAPHS", "0")
    eager = engine()
    assert not eager.runner.enable_graphs
    assert [generate(eager, p, 12, rid=f"r{i}") for i, p in enumerate(prompts)] \
        == with_graphs
