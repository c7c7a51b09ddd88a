"""Shared helpers of the int4 tests: AWQ-gemm packing, a synthetic AWQ
checkpoint, the fp64 oracle and the derived error bound."""
import json
import os

import torch

from kubeai_amd.models.loader import _REVERSE_AWQ_ORDER


def awq_pack_cols(m: torch.Tensor) -> torch.Tensor:
    """int [r, c] nibbles in logical column order -> AWQ-gemm int32 [r, c/8]."""
    inv = [0] * 8
    for shift_i, logical in enumerate(_REVERSE_AWQ_ORDER):
        inv[logical] = shift_i
    r, c = m.shape
    m = m.to(torch.int64).view(r, c // 8, 8)
    out = torch.zeros(r, c // 8, dtype=torch.int64)
    for logical in range(8):
        out |= m[:, :, logical] << (4 * inv[logical])
    out = torch.where(out >= 2**31, out - 2**32, out)
    return out.to(torch.int32)


def random_awq(N: int, K: int, g: int, seed: int = 0):
    """Random AWQ-gemm tensors (qweight [K, N/8], qzeros [K/g, N/8], scales
    fp16 [K/g, N]) together with their logical codes (q [N, K] uint8,
    z [N, K/g] uint8, s [N, K/g] fp16)."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 16, (N, K), generator=gen, dtype=torch.uint8)
    z = torch.randint(0, 16, (N, K // g), generator=gen, dtype=torch.uint8)
    s = (torch.rand(N, K // g, generator=gen) * 0.02 + 0.001).half()
    return (
        awq_pack_cols(q.t().contiguous()),
        awq_pack_cols(z.t().contiguous()),
        s.t().contiguous(),
        (q, z, s),
    )


def dequant_formula(q, z, s, g: int) -> torch.Tensor:
    """w[n, k] = bf16_rne(float(q - z) * float(s)), written out directly."""
    zf = z.float().repeat_interleave(g, dim=1)
    sf = s.float().repeat_interleave(g, dim=1)
    return ((q.float() - zf) * sf).to(torch.bfloat16)


def awq_quantize(weight: torch.Tensor, group: int):
    """Min/max round-to-nearest, the arithmetic of awq_pack in
    test_weight_loading.py: weight [out, in] -> (qweight, qzeros, scales)."""
    w = weight.float().t().contiguous()  # [in, out]
    i, o = w.shape
    wg = w.view(i // group, group, o)
    mn = wg.min(dim=1).values
    mx = wg.max(dim=1).values
    scale = torch.clamp((mx - mn) / 15.0, min=1e-8)
    zero = torch.round(-mn / scale).clamp(0, 15)
    q = torch.round(wg / scale.unsqueeze(1) + zero.unsqueeze(1)).clamp(0, 15)
    return (
        awq_pack_cols(q.to(torch.int32).view(i, o)),
        awq_pack_cols(zero.to(torch.int32)),
        scale.half(),
    )


def write_awq_checkpoint(model, out_dir, group: int = 64, pack=None) -> str:
    """Save `model` in HF layout with every decoder projection AWQ-packed.
    pack(name) -> bool narrows which 2-D projection tensors are packed."""
    from safetensors.torch import load_file, save_file

    from kubeai_amd.models.loader import save_hf_checkpoint

    out_dir = str(out_dir)
    bf16_dir = out_dir + "_bf16"
    save_hf_checkpoint(model, bf16_dir)
    tensors = load_file(os.path.join(bf16_dir, "model.safetensors"))
    out = {}
    for k, v in tensors.items():
        is_proj = (
            k.endswith(".weight") and v.dim() == 2 and "norm" not in k
            and "embed" not in k and "lm_head" not in k
            and ".gate.weight" not in k  # MoE router stays float
        )
        if is_proj and (pack is None or pack(k)):
            qw, qz, sc = awq_quantize(v, group)
            pre = k[: -len(".weight")]
            out[pre + ".qweight"], out[pre + ".qzeros"] = qw, qz
            out[pre + ".scales"] = sc
        else:
            out[k] = v
    os.makedirs(out_dir, exist_ok=True)
    save_file(out, os.path.join(out_dir, "model.safetensors"))
    with open(os.path.join(bf16_dir, "config.json")) as f:
        cfg = json.load(f)
    cfg["quantization_config"] = {
        "quant_method": "awq", "bits": 4, "group_size": group, "version": "gemm",
    }
    with open(os.path.join(out_dir, "config.json"), "w") as f:
        json.dump(cfg, f)
    return out_dir


def generate(eng, prompt, n: int, rid: str = "r"):
    from kubeai_amd.engine import SamplingParams

    eng.add_request(
        prompt, SamplingParams(max_tokens=n, ignore_eos=True), request_id=rid
    )
    for _ in range(20 * n + 50):
        if not eng.has_work():
            break
        for o in eng.step():
            if o.finished:
                return o.output_token_ids
    raise AssertionError("did not finish")


# ---------------------------------------------------------------- the bound
def oracle(x: torch.Tensor, w_deq: torch.Tensor):
    """fp64 reference and the magnitude sum A = |x| @ |W|^T."""
    xd, wd = x.double().cpu(), w_deq.double().cpu()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def bound(ref: torch.Tensor, A: torch.Tensor, K: int, out_ulp: float = 2.0**-9):
    """|y - ref| <= 2 * (out_ulp * |ref| + K * 2^-24 * A) + 1e-6.

    bf16 x bf16 products are exact in fp32; K fp32 additions in any order
    contribute at most K * 2^-24 * A; rounding the result to bf16 contributes
    2^-9 * |ref|; the sum is doubled, as in the attention bound."""
    return 2.0 * (out_ulp * ref.abs() + K * 2.0**-24 * A) + 1e-6


def assert_within_bound(y, x, w_deq, out_ulp: float = 2.0**-9, what: str = ""):
    ref, A = oracle(x, w_deq)
    err = (y.double().cpu() - ref).abs()
    lim = bound(ref, A, x.shape[1], out_ulp)
    worst = (err / lim).max().item()
    print(f"int4 bound {what}: max err/bound = {worst:.4f}")
    assert bool((err <= lim).all()), f"{what}: err/bound = {worst}"
