"""int4 (AWQ W4A16) serving, CPU side: the weight format and its torch
reference, the packed checkpoint load, conversion, the public flag, and a
self-check of the error bound the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

from int4_util import (
    assert_within_bound, awq_quantize, dequant_formula, generate, random_awq,
    write_awq_checkpoint,
)
from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine
from kubeai_amd.engine.quant_int4 import Int4Linear, Int4Weight, convert_to_int4
from kubeai_amd.models.loader import _awq_dequant


def make_engine(model, **kw):
    kw.setdefault("seed", 3)
    return LLMEngine(
        EngineConfig(model=model, device="cpu", num_gpu_blocks=128,
                     max_model_len=512, **kw)
    )


# ------------------------------------------------------------ weight format
@pytest.mark.parametrize("g", [32, 64, 128])
def test_from_awq_matches_awq_dequant(g):
    qw, qz, sc, _ = random_awq(48, 256, g, seed=g)
    w = Int4Weight.from_awq(qw, qz, sc)
    assert (w.N, w.K, w.group) == (48, 256, g)
    assert torch.equal(w.dequant(), _awq_dequant(qw, qz, sc))
    assert torch.equal(ops.int4_dequant(w), w.dequant())


@pytest.mark.parametrize("g,K", [(32, 160), (64, 256), (128, 384)])
def test_from_codes_matches_formula(g, K):
    # K = 160 and 384 leave the last 128-chunk of the packing ragged
    _, _, _, (q, z, s) = random_awq(32, K, g, seed=1)
    w = Int4Weight.from_codes(q, z, s)
    assert torch.equal(w.dequant(), dequant_formula(q, z, s, g))
    q2, z2, s2 = w.codes()
    assert torch.equal(q2.to(torch.uint8), q)
    assert torch.equal(z2.to(torch.uint8), z) and torch.equal(s2, s)
    G = K // g
    assert w.nbytes == 32 * (-(-K // 128) * 128) // 2 + 32 * G * 2 + 32 * G // 2


def test_cat_equals_cat_of_dequants():
    ws = [
        Int4Weight.from_codes(*random_awq(n, 256, 64, seed=n)[3])
        for n in (32, 16, 48)
    ]
    joined = Int4Weight.cat(ws)
    assert joined.N == 96
    assert torch.equal(joined.dequant(), torch.cat([w.dequant() for w in ws]))
    with pytest.raises(ValueError):
        Int4Weight.cat(
            [ws[0], Int4Weight.from_codes(*random_awq(16, 128, 64)[3])]
        )


@pytest.mark.parametrize("g", [32, 64, 128])
def test_quantize_rtn_half_step(g):
    torch.manual_seed(g)
    w = torch.randn(32, 512).to(torch.bfloat16)
    q = Int4Weight.quantize_rtn(w, g)
    _, _, s = q.codes()
    step = s.float().repeat_interleave(g, dim=1)
    err = (q.dequant().float() - w.float()).abs()
    # half a step from rounding the code (the rounded zero point keeps min and
    # max inside the clamp to within that half step), plus the two number
    # formats: the fp16 rounding of the step (2^-11 relative, times a code
    # distance of at most 15) and the bf16 rounding of the result
    lim = 0.5 * step + 15 * step * 2.0**-11 + w.float().abs() * 2.0**-8
    assert bool((err <= lim).all()), (err / lim).max()


def test_shape_rules_raise():
    _, _, _, (q, z, s) = random_awq(16, 96, 32)
    with pytest.raises(ValueError):  # K % g != 0
        Int4Weight.quantize_rtn(torch.randn(16, 96), 64)
    with pytest.raises(ValueError):  # N % 16 != 0
        Int4Weight.from_codes(q[:8], z[:8], s[:8])
    with pytest.raises(ValueError):  # g = 16
        Int4Weight.quantize_rtn(torch.randn(16, 96), 16)


def test_int4_linear_module():
    torch.manual_seed(0)
    lin = torch.nn.Linear(128, 32, bias=True).to(torch.bfloat16)
    q = Int4Linear(Int4Weight.quantize_rtn(lin.weight, 32), lin.bias)
    assert not hasattr(q, "forward_quantized")
    x = torch.randn(5, 128).to(torch.bfloat16)
    assert q.weight.dtype == torch.bfloat16 and q.weight.shape == (32, 128)
    assert torch.equal(q(x), F.linear(x, q.weight) + lin.bias)


# ------------------------------------------------------------------ engine
def int4_bytes(model):
    n = 0
    for m in model.modules():
        if isinstance(m, Int4Linear):
            n += sum(b.numel() * b.element_size() for b in m.buffers())
    return n


def test_awq_checkpoint_served_packed(tmp_path):
    """The packed load serves exactly the checkpoint's codes: on CPU both
    loads compute F.linear over the same bf16 weights, so greedy tokens are
    identical."""
    src = make_engine("llama-tiny")
    ckpt = write_awq_checkpoint(src.runner.model, tmp_path / "awq", group=64)
    dense = make_engine(ckpt, seed=999)
    packed = make_engine(ckpt, seed=999, quantization="int4")
    prompt = list(range(10, 60))
    assert generate(packed, prompt, 8) == generate(dense, prompt, 8)

    model = packed.runner.model
    bf16_bytes = 0
    for layer, ref_layer in zip(model.layers, dense.runner.model.layers):
        for mod, ref_mod in ((layer.self_attn, ref_layer.self_attn),
                             (layer.mlp, ref_layer.mlp)):
            for name in ("qkv_proj", "o_proj", "gate_up_proj", "down_proj"):
                lin = getattr(mod, name, None)
                if lin is None:
                    continue
                assert isinstance(lin, Int4Linear), name
                assert lin.group == 64
                ref_w = getattr(ref_mod, name).weight
                # no re-quantization: the checkpoint's own dequantization
                assert torch.equal(lin.weight, ref_w)
                bf16_bytes += ref_w.numel() * 2
    assert bf16_bytes > 0
    assert int4_bytes(model) <= 0.30 * bf16_bytes
    assert isinstance(model.lm_head, torch.nn.Linear)
    assert model.lm_head.weight.dtype == torch.bfloat16


def test_float_weights_convert(tmp_path):
    eng = make_engine("llama-tiny", quantization="int4")
    model = eng.runner.model
    assert isinstance(model.layers[0].self_attn.qkv_proj, Int4Linear)
    assert model.layers[0].self_attn.qkv_proj.group == 128
    assert isinstance(model.lm_head, torch.nn.Linear)
    assert len(generate(eng, list(range(10, 40)), 4)) == 4


def test_mixtral_convert_generates():
    eng = make_engine("mixtral-tiny")
    n = convert_to_int4(eng.runner.model)
    mlp = eng.runner.model.layers[0].mlp
    assert isinstance(mlp.experts[0].gate_up_proj, Int4Linear)
    assert isinstance(mlp.experts[-1].down_proj, Int4Linear)
    assert isinstance(mlp.gate, torch.nn.Linear)  # the router stays float
    n_layers = len(eng.runner.model.layers)
    assert n == n_layers * (2 + 2 * len(mlp.experts))
    assert len(generate(eng, list(range(10, 40)), 4)) == 4


def test_tp_group_raises():
    from kubeai_amd.engine.runner import ModelRunner
    from kubeai_amd.models.config import PRESETS

    with pytest.raises(NotImplementedError, match="tensor"):
        ModelRunner(PRESETS["llama-tiny"], device="cpu", num_gpu_blocks=16,
                    quantization="int4", tp_group=object())
    from kubeai_amd.models.loader import load_weights_tp

    with pytest.raises(NotImplementedError):
        load_weights_tp(None, "unused", keep_int4=True)


def test_packed_moe_checkpoint_raises(tmp_path):
    src = make_engine("mixtral-tiny")
    ckpt = write_awq_checkpoint(src.runner.model, tmp_path / "moe", group=64)
    with pytest.raises(NotImplementedError, match="MoE"):
        make_engine(ckpt, quantization="int4")


def test_unsupported_group_names_layer(tmp_path):
    """An unsupported group size or a K that is no multiple of it is a
    ValueError that says which layer, from conversion and from the packed
    load alike."""
    eng = make_engine("llama-tiny")
    ckpt = write_awq_checkpoint(eng.runner.model, tmp_path / "g16", group=16)
    with pytest.raises(ValueError, match=r"layers\.0\.\w+\.\w+_proj.*group"):
        make_engine(ckpt, quantization="int4")
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.qkv_proj"):
        convert_to_int4(eng.runner.model, group=48)
    lin = torch.nn.Linear(96, 16, bias=False)
    holder = torch.nn.Module()
    holder.o_proj = lin
    with pytest.raises(ValueError, match="o_proj"):  # K % g != 0
        convert_to_int4(holder, group=64)


def test_cli_flag_parses():
    from kubeai_amd.engine.server import build_arg_parser

    args = build_arg_parser().parse_args(
        ["--model", "llama-tiny", "--quantization", "int4"]
    )
    assert args.quantization == "int4"


def test_catalog_has_int4_entry():
    import os

    import yaml

    path = os.path.join(os.path.dirname(__file__), "..", "deploy", "models",
                        "catalog.yaml")
    with open(path) as f:
        catalog = yaml.safe_load(f)["catalog"]
    hits = [
        name for name, spec in catalog.items()
        if list(spec.get("args") or [])[-2:] == ["--quantization", "int4"]
    ]
    assert hits, "no catalog entry passes --quantization int4"


# ------------------------------------------------- the GPU tests' bound
def _bound_case(g=64, N=48, K=512, M=33):
    _, _, _, (q, z, s) = random_awq(N, K, g, seed=7)
    torch.manual_seed(11)
    x = torch.randn(M, K).to(torch.bfloat16)
    return x, (q, z, s), dequant_formula(q, z, s, g)


def _bf16_linear(x, w):
    return F.linear(x.float(), w.float()).to(torch.bfloat16)


@pytest.mark.parametrize("g", [32, 64, 128])
def test_bound_accepts_fp32_linear(g):
    x, _, w = _bound_case(g)
    assert_within_bound(_bf16_linear(x, w), x, w, what=f"fp32 linear g={g}")


@pytest.mark.parametrize("mutant", ["group_off_by_one", "nibble_swap", "no_zero"])
def test_bound_rejects_mutants(mutant):
    g = 64
    x, (q, z, s), w = _bound_case(g)
    if mutant == "group_off_by_one":
        bad = dequant_formula(q, z.roll(1, dims=1), s.roll(1, dims=1), g)
    elif mutant == "nibble_swap":
        bad = dequant_formula(
            q.view(q.shape[0], -1, 2).flip(-1).reshape(q.shape), z, s, g
        )
    else:
        bad = dequant_formula(q, torch.zeros_like(z), s, g)
    with pytest.raises(AssertionError):
        assert_within_bound(_bf16_linear(x, bad), x, w, what=mutant)
