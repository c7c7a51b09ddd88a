"""MXFP4 format (engine/quant_mxfp4.py) on CPU: packing round trips, the
dequantization formula, round-to-nearest quantization on hand-worked blocks,
and a tiny engine."""
import pytest
import torch

from int4_util import generate
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_mxfp4 import (
    E2M1_VALUES, Mxfp4Linear, Mxfp4Weight,
)

GRID = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES))


def random_codes(N, K, seed=0, e_lo=120, e_hi=134):
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=gen, dtype=torch.uint8)
    scales = torch.randint(e_lo, e_hi + 1, (N, K // 32), generator=gen, dtype=torch.uint8)
    return codes, scales


def formula(codes, scales):
    """w[n, k] = e2m1(code) * 2^(e - 127) in fp64, low nibble = even k."""
    nib = torch.stack([codes & 0xF, codes >> 4], dim=-1).flatten(1)
    e = scales.double().repeat_interleave(32, dim=1)
    return GRID.double()[nib.long()] * torch.pow(2.0, e - 127)


# K = 160 and 2208 have a padded last chunk; 4256 needs two scale words per lane
@pytest.mark.parametrize("N,K", [(16, 128), (48, 160), (32, 2208), (16, 4256)])
def test_round_trip_and_dequant(N, K):
    codes, scales = random_codes(N, K, seed=K)
    w = Mxfp4Weight.from_codes(codes, scales)
    back = w.codes()
    assert torch.equal(back[0], codes) and torch.equal(back[1], scales)
    assert w.nbytes >= N * K // 2 + N * K // 32
    deq = w.dequant()
    assert deq.dtype == torch.bfloat16 and deq.shape == (N, K)
    assert torch.equal(deq.double(), formula(codes, scales))


def test_dequant_all_codes_by_hand():
    """One block holds every code twice; exponents at both accepted ends."""
    block = torch.arange(16, dtype=torch.uint8).repeat(2)          # k -> code k % 16
    codes = (block[0::2] | (block[1::2] << 4)).repeat(16, 1)       # [16, 16]
    for e in (2, 127, 130, 252):
        w = Mxfp4Weight.from_codes(codes, torch.full((16, 1), e, dtype=torch.uint8))
        want = (GRID.double().repeat(2) * 2.0 ** (e - 127)).repeat(16, 1)
        got = w.dequant()
        assert torch.equal(got.double(), want), e
        assert torch.equal(torch.signbit(got[0]), block >= 8)      # -0 keeps its sign


def test_quantize_rtn_by_hand():
    w = torch.zeros(16, 128)
    # block 0: amax = 6 * 2^3 -> X = floor(log2 48) - 2 = 3, e = 130
    w[0, :8] = torch.tensor([48.0, -24.0, 4.0, 12.0, 0.0, 8.0, -32.0, 16.0])
    # block 1 stays all zero -> e = 127, zero codes
    # block 2: amax = 4 -> X = 0; ties go to the even code: 0.25 -> 0,
    # 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4; 2.6 -> 3 is no tie
    w[0, 64:72] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, -2.5, 3.5, 2.6])
    # block 3: amax = 7.9 -> X = 0, 7.9 and -7 saturate at +-6, 5 ties to 4
    w[0, 96:100] = torch.tensor([7.9, -7.0, 5.0, 5.1])
    q = Mxfp4Weight.quantize_rtn(w)
    codes, scales = q.codes()
    assert scales[0].tolist() == [130, 127, 127, 127]
    assert scales[1:].eq(127).all() and codes[1:].eq(0).all()
    deq = q.dequant().float()
    assert deq[0, :8].tolist() == [48.0, -24.0, 4.0, 12.0, 0.0, 8.0, -32.0, 16.0]
    assert deq[0, 32:64].eq(0).all()
    assert deq[0, 64:72].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, -2.0, 4.0, 3.0]
    assert deq[0, 96:100].tolist() == [6.0, -6.0, 4.0, 6.0]
    # exponents clamp into the accepted range
    tiny = Mxfp4Weight.quantize_rtn(torch.full((16, 32), 2.0 ** -140))
    assert tiny.codes()[1].eq(2).all()


def test_cat_equals_packing_the_concatenation():
    a, b = random_codes(32, 2208, seed=1), random_codes(16, 2208, seed=2)
    joined = Mxfp4Weight.cat([Mxfp4Weight.from_codes(*a), Mxfp4Weight.from_codes(*b)])
    whole = Mxfp4Weight.from_codes(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
    assert (joined.N, joined.K) == (48, 2208)
    assert torch.equal(joined.qp, whole.qp) and torch.equal(joined.sp, whole.sp)
    with pytest.raises(ValueError):
        Mxfp4Weight.cat([whole, Mxfp4Weight.from_codes(*random_codes(16, 128))])


@pytest.mark.parametrize("codes_shape,scales_shape,e", [
    ((16, 64), (16, 4), 255),   # NaN scale
    ((16, 64), (16, 4), 253),   # 6 * 2^126 overflows bf16
    ((16, 64), (16, 4), 1),     # 0.5 * 2^-126 is a bf16 subnormal
    ((24, 64), (24, 4), 127),   # N % 16
    ((16, 72), (16, 4), 127),   # codes and scales disagree on K
    ((16, 64), (32, 4), 127),   # ... and on N
])
def test_from_codes_rejects(codes_shape, scales_shape, e):
    with pytest.raises(ValueError):
        Mxfp4Weight.from_codes(
            torch.zeros(codes_shape, dtype=torch.uint8),
            torch.full(scales_shape, e, dtype=torch.uint8),
        )


def test_convert_marks_only_layers_the_fused_branch_serves():
    """SwiGLU layers without a residual multiplier are marked; granite
    (residual_multiplier) and GeGLU layers keep the bf16 branch."""
    from kubeai_amd.engine.quant_mxfp4 import convert_to_mxfp4
    from kubeai_amd.models.config import PRESETS
    from kubeai_amd.models.llama import LlamaForCausalLM

    for preset, marked in [("llama-tiny", True), ("granite-tiny", False),
                           ("gemma-tiny", False)]:
        model = LlamaForCausalLM(PRESETS[preset])
        assert convert_to_mxfp4(model) == 4 * len(model.layers)
        for layer in model.layers:
            assert getattr(layer, "_mxfp4_fused", False) is marked, preset


def test_engine_cpu():
    def engine():
        return LLMEngine(EngineConfig(
            model="llama-tiny", device="cpu", num_gpu_blocks=64,
            max_model_len=256, seed=3, quantization="mxfp4",
        ))

    eng = engine()
    layer = eng.runner.model.layers[0]
    assert isinstance(layer.self_attn.qkv_proj, Mxfp4Linear)
    assert isinstance(layer.mlp.down_proj, Mxfp4Linear)
    assert not isinstance(eng.runner.model.lm_head, Mxfp4Linear)
    out = generate(eng, list(range(10, 30)), 4)
    assert len(out) == 4 and out == generate(engine(), list(range(10, 30)), 4)
