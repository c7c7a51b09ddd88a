"""FP8 (OCP e4m3fn) weight + dynamic per-token activation quantization.

MI355X-first: gfx950's fp8 MFMA peak is ~2x bf16 and — what actually
matters for skinny decode GEMMs — fp8 weights halve the HBM bytes per
step. The BASELINE headline config is Llama-3.1-8B-Instruct-FP8, so this
is the config-faithful serving mode. GEMMs go through torch._scaled_mm
(hipBLASLt fp8 path); gfx950 uses OCP e4m3fn, not the MI300X fnuz variant.

Scheme: W8A8 dynamic — per-output-channel weight scales, per-token
activation scales (amax/448), bf16 output.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from kubeai_amd import ops

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0


class Fp8Linear(nn.Module):
    """Drop-in replacement for bias-free nn.Linear, fp8 weights."""

    def __init__(self, weight_bf16: torch.Tensor, bias: torch.Tensor | None = None):
        super().__init__()
        if bias is not None:
            self.register_buffer("bias", bias.detach().to(torch.bfloat16))
        else:
            self.bias = None
        w = weight_bf16.detach().float()
        w_amax = w.abs().amax(dim=1, keepdim=True).clamp_min(1e-6)  # [out,1]
        w_scale = w_amax / FP8_MAX
        wq = (w / w_scale).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
        # scaled_mm wants mat2 column-major: keep [out, in] row-major and
        # pass .t() (a column-major view) at call time
        self.register_buffer("weight_fp8", wq.contiguous())
        self.register_buffer("weight_scale", w_scale.reshape(1, -1).contiguous())
        self.out_features, self.in_features = weight_bf16.shape

    @property
    def weight(self) -> torch.Tensor:
        """bf16 view for code paths that read .weight (LoRA base, tests)."""
        return (
            self.weight_fp8.float() * self.weight_scale.reshape(-1, 1)
        ).to(torch.bfloat16)

    def forward_quantized(self, xq: torch.Tensor, x_scale: torch.Tensor) -> torch.Tensor:
        """Pre-quantized input from a fused producer kernel (quant is free)."""
        if not xq.is_cuda:
            # CPU semantics fallback (tests): dequantize and matmul
            x = xq.float() * x_scale.view(-1, 1)
            w = self.weight_fp8.float() * self.weight_scale.reshape(-1, 1)
            y = (x @ w.t()).to(torch.bfloat16)
            return y + self.bias if self.bias is not None else y
        return torch._scaled_mm(
            xq,
            self.weight_fp8.t(),
            scale_a=x_scale.view(-1, 1),
            scale_b=self.weight_scale,
            bias=self.bias,
            out_dtype=torch.bfloat16,
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # scale = max(amax, 1e-6) / 448, q = e4m3(clamp(x / scale, ±448)):
        # the division form, which rounds differently from the fused
        # producers' x * (448 / amax). One launch for 2-D contiguous bf16 on
        # GPU, the torch chain (byte-equal to it) for everything else.
        xq, a_scale = ops.quant_fp8_div(x)
        if not x.is_cuda:
            return self.forward_quantized(xq, a_scale.squeeze(-1))
        return torch._scaled_mm(
            xq,
            self.weight_fp8.t(),
            scale_a=a_scale,
            scale_b=self.weight_scale,
            bias=self.bias,
            out_dtype=torch.bfloat16,
        )


class Fp8ExpertGroup:
    """The E Fp8Linears of one MoE projection (every expert's gate_up_proj,
    or every expert's down_proj) as the grouped kernel (csrc/fp8_moe.hip)
    takes them: the modules themselves, not a copy of their weights, and
    `table`, an int64 [E, 2] tensor on their device holding each expert's
    (weight_fp8, weight_scale) address.

    All experts share N, K and device and have no bias. The table is built
    here, when the experts are converted or moved; ops.fp8_moe_linear only
    reads it (that call can run under graph capture, where building it would
    be a host-to-device copy inside the capture)."""

    def __init__(self, linears: list[Fp8Linear]):
        if not linears:
            raise ValueError("fp8 expert group: no experts")
        for e, lin in enumerate(linears):
            if not isinstance(lin, Fp8Linear):
                raise ValueError(
                    f"fp8 expert group: expert {e} is a "
                    f"{type(lin).__name__}, not an Fp8Linear"
                )
            if lin.bias is not None:
                raise ValueError(f"fp8 expert group: expert {e} has a bias")
        w0 = linears[0].weight_fp8
        for e, lin in enumerate(linears):
            w, s = lin.weight_fp8, lin.weight_scale
            if w.dim() != 2 or w.shape != w0.shape or s.numel() != w.shape[0]:
                raise ValueError(
                    f"fp8 expert group: expert {e} is {list(w.shape)} with "
                    f"{s.numel()} scales, expert 0 is {list(w0.shape)}"
                )
            if w.dtype != FP8_DTYPE or s.dtype != torch.float32:
                raise ValueError(
                    f"fp8 expert group: expert {e} holds {w.dtype} weights "
                    f"and {s.dtype} scales, need {FP8_DTYPE} and float32"
                )
            if w.device != w0.device or s.device != w0.device:
                raise ValueError(
                    f"fp8 expert group: expert {e} is on {w.device} (scales "
                    f"on {s.device}), expert 0 on {w0.device}"
                )
            if not (w.is_contiguous() and s.is_contiguous()) or w.data_ptr() % 16:
                raise ValueError(
                    f"fp8 expert group: expert {e}'s weight and scales must "
                    "be contiguous and the weight 16-byte aligned"
                )
        self.linears = list(linears)
        # the tensors the table points at: holds() compares against these
        self._tensors = [(lin.weight_fp8, lin.weight_scale) for lin in linears]
        self.E = len(linears)
        self.N, self.K = w0.shape
        self.table = torch.tensor(
            [[w.data_ptr(), s.data_ptr()] for w, s in self._tensors],
            dtype=torch.int64,
        ).to(w0.device)

    @property
    def device(self):
        return self._tensors[0][0].device

    def table_on(self, device) -> torch.Tensor:
        if self.table.device != device:
            raise RuntimeError(
                f"fp8 expert group lives on {self.table.device}, the call "
                f"is on {device}"
            )
        return self.table

    def holds(self, modules) -> bool:
        """Whether the group still describes exactly these modules' buffers
        (a buffer that was replaced leaves the table stale)."""
        return len(modules) == self.E and all(
            isinstance(lin, Fp8Linear)
            and w is lin.weight_fp8 and s is lin.weight_scale
            for (w, s), lin in zip(self._tensors, modules)
        )


def fp8_expert_groups(experts):
    """(gate_up group, down group) of a list of expert MLPs when every
    projection is a bias-free Fp8Linear, else None."""
    gate_up = [getattr(ex, "gate_up_proj", None) for ex in experts]
    down = [getattr(ex, "down_proj", None) for ex in experts]
    for lin in gate_up + down:
        if not isinstance(lin, Fp8Linear) or lin.bias is not None:
            return None
    return Fp8ExpertGroup(gate_up), Fp8ExpertGroup(down)


_TARGETS = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj", "lm_head")


def convert_to_fp8(model: nn.Module) -> int:
    """Swap target nn.Linear modules for Fp8Linear; returns count.

    Dense decoder layers additionally get the FUSED activation-quant path
    (llama.DecoderLayer checks _fp8_fused): producer kernels emit fp8 +
    per-row scales, so per-linear dynamic quantization disappears.
    """
    n = 0
    for mod in model.modules():
        for name in _TARGETS:
            child = getattr(mod, name, None)
            if isinstance(child, nn.Linear):
                setattr(mod, name, Fp8Linear(child.weight, child.bias))
                n += 1
    for layer in getattr(model, "layers", []):
        attn = getattr(layer, "self_attn", None)
        mlp = getattr(layer, "mlp", None)
        if attn is None or not isinstance(getattr(attn, "qkv_proj", None), Fp8Linear):
            continue
        if isinstance(getattr(mlp, "gate_up_proj", None), Fp8Linear):
            layer._fp8_fused = True  # dense: norms/activations emit fp8
        elif hasattr(mlp, "experts"):
            # MoE: attention runs the fused-fp8 path; the MLP input stays
            # bf16 (router needs it) and MoEMLP quantizes once itself
            layer._fp8_fused = True
    # MoE blocks: the grouped kernel's address tables, built now that every
    # expert is in place
    for mod in model.modules():
        refresh = getattr(mod, "refresh_fp8_groups", None)
        if refresh is not None:
            refresh()
    return n
