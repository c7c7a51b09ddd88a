"""MXFP4 (OCP microscaling FP4, W4A8) weights served as MXFP4.

e2m1 codes with one E8M0 scale byte per (output row, block of 32 consecutive
input columns): 4.25 bits per weight in HBM. Decode GEMMs
(M <= ops.MXFP4_M_FUSED) multiply the packed weight by e4m3 activations inside
gfx950's scaled matrix instruction (csrc/mxfp4_gemm.hip): there is no
dequantization step at all, and the activations are the (e4m3 rows, fp32 row
scale) pairs that the fused norm, activation and attention-merge kernels
already emit. Larger M dequantize into the shared bf16 workspace and run the
library GEMM, unless KUBEAI_MXFP4_TILED_M raises ops.mxfp4_m_max(): steps of up
to that many rows then stay on the scaled MFMA, in the output-tiled kernel
(csrc/mxfp4_gemm_tiled.hip).

The pinned semantics (OCP MX v1.0): an e2m1 code (sign, 2 exponent bits, 1
mantissa bit) is one of +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, and

    w[n, k] = e2m1(code[n, k]) * 2^(e[n, k // 32] - 127)

`Mxfp4Weight.dequant()` is the torch reference; the dequant kernel reproduces
it bit for bit and the fused kernel multiplies exactly these values.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from kubeai_amd import ops

BLOCK = 32    # k per E8M0 scale
_CHUNK = 128  # k per packed chunk (4 lanes x 32 codes), see mxfp4_gemm.hip
_WAVES = 8    # the kernel's K-split; the scale layout is built on it
# Accepted E8M0 bytes. Within them every nonzero weight, from 0.5 * 2^-125 to
# 6 * 2^125, is a normal bf16, so dequant() is exact; 255 is NaN.
E_MIN, E_MAX = 2, 252

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _n_groups(kc: int) -> int:
    """Scale words per (tile, wave, lane): one per 4 chunks of a wave's walk."""
    return ((kc + _WAVES - 1) // _WAVES + 3) // 4


class Mxfp4Weight:
    """One linear's quantized weight, logical [N, K], N % 16 == 0, K % 32 == 0.

    Physical packing (private to this class and csrc/mxfp4_gemm.hip; built
    once, here). N is cut into tiles of 16 rows, K into chunks of 128 with
    the last chunk padded with zero codes:

      qp uint8 [N/16, Kc, 64, 16]   unit kq*16 + nl holds the 32 consecutive-k
                                    codes (one MX block) of row tile*16 + nl
                                    from k = chunk*128 + kq*32, two per byte,
                                    low nibble = even k (one 16-byte lane load)
      sp uint8 [N/16, J, 8, 64, 4]  word (j, w, unit), byte c: the scale of
                                    that unit in chunk 32*j + 8*c + w, 127
                                    where the weight has no such chunk. Wave w
                                    of the kernel walks chunks w, w + 8, ...:
                                    one 4-byte load serves four of its steps

    Both are tile-major, so concatenation along N is a plain cat.
    """

    def __init__(self, qp, sp, N: int, K: int):
        self.qp, self.sp = qp, sp
        self.N, self.K = int(N), int(K)
        if qp.is_cuda:
            # the large-M route dequantizes into a process-wide workspace;
            # sized here, when the weight is built, never at call time
            ops.int4_reserve_workspace(qp.device, self.N * self.K)

    # ---------------------------------------------------------------- build
    @staticmethod
    def check_shape(N: int, K: int) -> None:
        if N <= 0 or K <= 0 or N % 16 or K % BLOCK:
            raise ValueError(
                f"mxfp4: weight [{N}, {K}] needs N % 16 == 0 and K % 32 == 0"
            )

    @classmethod
    def from_codes(cls, codes: torch.Tensor, scales: torch.Tensor):
        """codes uint8 [N, K/2]: two e2m1 codes per byte, low nibble = even k
        (the published checkpoint convention); scales uint8 [N, K/32]: E8M0,
        accepted in [2, 252], where every weight is a normal bf16 and
        dequant() therefore exact (255 is NaN; 0, 1, 253 and 254 would need
        bf16 subnormals or overflow)."""
        if (
            codes.dim() != 2 or scales.dim() != 2
            or codes.dtype != torch.uint8 or scales.dtype != torch.uint8
            or codes.shape[0] != scales.shape[0]
            or codes.shape[1] != scales.shape[1] * (BLOCK // 2)
        ):
            raise ValueError(
                f"mxfp4: codes {tuple(codes.shape)} {codes.dtype} and scales "
                f"{tuple(scales.shape)} {scales.dtype} do not describe one "
                "weight (uint8 [N, K/2] and uint8 [N, K/32])"
            )
        N, K = codes.shape[0], codes.shape[1] * 2
        cls.check_shape(N, K)
        if scales.numel() and (int(scales.min()) < E_MIN or int(scales.max()) > E_MAX):
            raise ValueError(
                f"mxfp4: scale bytes must lie in [{E_MIN}, {E_MAX}], got "
                f"[{int(scales.min())}, {int(scales.max())}]"
            )
        dev = codes.device
        kc = (K + _CHUNK - 1) // _CHUNK
        J = _n_groups(kc)
        cc = torch.zeros((N, kc * 64), dtype=torch.uint8, device=dev)
        cc[:, : K // 2] = codes
        # [tile, nl, chunk, kq, byte] -> [tile, chunk, kq, nl, byte]
        qp = (
            cc.view(N // 16, 16, kc, 4, 16).permute(0, 2, 3, 1, 4)
            .reshape(N // 16, kc, 64, 16).contiguous()
        )
        ss = torch.full((N, J * 32 * 4), 127, dtype=torch.uint8, device=dev)
        ss[:, : K // BLOCK] = scales
        # chunk = 32 j + 8 c + w: [tile, nl, j, c, w, kq] -> [tile, j, w, kq, nl, c]
        sp = (
            ss.view(N // 16, 16, J, 4, _WAVES, 4).permute(0, 2, 4, 5, 1, 3)
            .reshape(N // 16, J, _WAVES, 64, 4).contiguous()
        )
        return cls(qp, sp, N, K)

    @classmethod
    def quantize_rtn(cls, weight: torch.Tensor):
        """Round-to-nearest per block: X = floor(log2(amax)) - 2 clamped to
        the accepted exponents, e = X + 127, element = w / 2^X rounded to the
        nearest e2m1 value, ties to the even code, saturating at +-6. An
        all-zero block gets e = 127 and zero codes."""
        N, K = weight.shape
        cls.check_shape(N, K)
        w = weight.detach().float().view(N, K // BLOCK, BLOCK)
        amax = w.abs().amax(dim=2)
        # frexp: amax = m * 2^ex with m in [0.5, 1), so floor(log2) = ex - 1
        X = torch.frexp(amax)[1] - 3
        X = torch.where(amax > 0, X, torch.zeros_like(X))
        X = X.clamp(E_MIN - 127, E_MAX - 127)
        v = torch.ldexp(w, -X.unsqueeze(2))  # exact: a power of two
        a = v.abs().clamp(max=6.0)
        step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
        q = torch.round(a / step) * step  # half to even on the grid's index
        # 2q in {0, 1, 2, 3, 4, 6, 8, 12} -> code 0..7
        lut = torch.tensor(
            [0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7], dtype=torch.uint8,
            device=w.device,
        )
        code = lut[(2 * q).long()] | (((v < 0) & (q > 0)).to(torch.uint8) << 3)
        code = code.view(N, K // 2, 2)
        return cls.from_codes(
            code[..., 0] | (code[..., 1] << 4), (X + 127).to(torch.uint8)
        )

    @classmethod
    def cat(cls, weights: list["Mxfp4Weight"]):
        """Concatenate along N (fused qkv, gate_up)."""
        w0 = weights[0]
        for w in weights[1:]:
            if w.K != w0.K:
                raise ValueError(
                    f"mxfp4: cannot join [{w.N}, {w.K}] with [{w0.N}, {w0.K}]"
                )
        return cls(
            torch.cat([w.qp for w in weights]),
            torch.cat([w.sp for w in weights]),
            sum(w.N for w in weights), w0.K,
        )

    # ----------------------------------------------------------------- read
    def codes(self):
        """(codes uint8 [N, K/2], scales uint8 [N, K/32]) in logical order."""
        N, K = self.N, self.K
        kc, J = self.qp.shape[1], self.sp.shape[1]
        codes = (
            self.qp.view(N // 16, kc, 4, 16, 16).permute(0, 3, 1, 2, 4)
            .reshape(N, kc * 64)[:, : K // 2]
        )
        scales = (
            self.sp.view(N // 16, J, _WAVES, 4, 16, 4).permute(0, 4, 1, 5, 2, 3)
            .reshape(N, J * 32 * 4)[:, : K // BLOCK]
        )
        return codes.contiguous(), scales.contiguous()

    def dequant(self) -> torch.Tensor:
        """bf16 [N, K], pure torch, any device: the reference."""
        codes, scales = self.codes()
        nib = torch.stack([codes & 0xF, codes >> 4], dim=-1).view(self.N, self.K)
        vals = torch.tensor(
            E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32,
            device=codes.device,
        )
        X = scales.to(torch.int32).repeat_interleave(BLOCK, dim=1) - 127
        return torch.ldexp(vals[nib.long()], X).to(torch.bfloat16)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.qp, self.sp))

    @property
    def device(self):
        return self.qp.device

    def to(self, device) -> "Mxfp4Weight":
        return Mxfp4Weight(self.qp.to(device), self.sp.to(device), self.N, self.K)


class Mxfp4Linear(nn.Module):
    """Drop-in replacement for nn.Linear over an Mxfp4Weight. Like Fp8Linear
    it has forward_quantized, which takes what the fp8 producer kernels emit."""

    def __init__(self, w: Mxfp4Weight, bias: torch.Tensor | None = None):
        super().__init__()
        self.register_buffer("qweight", w.qp)
        self.register_buffer("scales", w.sp)
        self.out_features, self.in_features = w.N, w.K
        # the bias Parameter object is kept as it is (a checkpoint load may
        # still fill it in place)
        self.bias = bias

    def _apply(self, fn, *args, **kwargs):
        # .to()/.cuda(): re-wrap the moved buffers now, so the workspace is
        # reserved at the move, not at the first forward
        super()._apply(fn, *args, **kwargs)
        self._w = None
        self.mxfp4
        return self

    @property
    def mxfp4(self) -> Mxfp4Weight:
        w = getattr(self, "_w", None)
        if w is None or w.qp is not self.qweight:
            w = self._w = Mxfp4Weight(
                self.qweight, self.scales, self.out_features, self.in_features
            )
        return w

    @property
    def weight(self) -> torch.Tensor:
        """Dequantized bf16 for code paths that read .weight (LoRA base,
        tests)."""
        return self.mxfp4.dequant()

    def forward_quantized(self, xq: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
        """Pre-quantized input from a fused producer kernel: e4m3 [M, K] and
        fp32 row scales, M <= ops.mxfp4_m_max() (the layer code sends no
        more)."""
        if xq.shape[0] > ops.mxfp4_m_max():
            raise RuntimeError(
                f"Mxfp4Linear.forward_quantized takes at most "
                f"{ops.mxfp4_m_max()} rows, got {xq.shape[0]}"
            )
        y = ops.mxfp4_linear(xq, xs, self.mxfp4)
        return y + self.bias if self.bias is not None else y

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 2:
            return self.forward(x.reshape(-1, x.shape[-1])).view(
                *x.shape[:-1], self.out_features
            )
        if not x.is_cuda:
            y = torch.nn.functional.linear(x, self.mxfp4.dequant())
        elif 1 <= x.shape[0] <= ops.mxfp4_m_max():
            y = ops.mxfp4_linear(*ops.quant_fp8(x.contiguous()), self.mxfp4)
        else:
            dense = ops.mxfp4_dequant(
                self.mxfp4,
                out=ops.dequant_workspace(
                    x.device, self.out_features, self.in_features
                ),
            )
            y = torch.nn.functional.linear(x, dense)
        return y + self.bias if self.bias is not None else y


_TARGETS = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj")


def convert_to_mxfp4(model: nn.Module) -> int:
    """Swap the target nn.Linear modules of a dense model for Mxfp4Linear,
    round-to-nearest; returns the count. lm_head stays bf16. Each decoder
    layer is marked so that steps of at most ops.mxfp4_m_max() rows take its
    fused-fp8 branch (llama.DecoderLayer.fp8_fused): norms, activation and
    attention merge emit e4m3 rows and the linears consume them as they are."""
    n = 0
    for mod_name, mod in model.named_modules():
        for name in _TARGETS:
            child = getattr(mod, name, None)
            if not isinstance(child, nn.Linear):
                continue
            try:
                w = Mxfp4Weight.quantize_rtn(child.weight)
            except ValueError as e:
                raise ValueError(f"{mod_name}.{name}: {e}") from None
            setattr(mod, name, Mxfp4Linear(w, child.bias))
            n += 1
    for layer in getattr(model, "layers", []):
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        # the fused branch's activation kernel is SwiGLU's, and it applies no
        # residual multiplier (granite): such layers keep the bf16 branch
        if (
            not getattr(mlp, "gelu", False)
            and getattr(layer, "res_mult", 1.0) == 1.0
        ) and all(
            isinstance(getattr(owner, name, None), Mxfp4Linear)
            for owner, name in (
                (attn, "qkv_proj"), (attn, "o_proj"),
                (mlp, "gate_up_proj"), (mlp, "down_proj"),
            )
        ):
            layer._mxfp4_fused = True
    return n
