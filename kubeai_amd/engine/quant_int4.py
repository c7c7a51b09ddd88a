"""INT4 (AWQ-style W4A16) weights served as int4.

Asymmetric 4-bit codes with one fp16 scale and one 4-bit zero point per
(output row, group of g input columns), g in {32, 64, 128}. The weight
stays packed in HBM (0.5 + 2.5/g bytes per weight instead of 2); decode
GEMMs (M <= ops.INT4_M_FUSED) dequantize in registers inside the fused
gfx950 kernel (csrc/int4_gemm.hip), larger M dequantize into a shared
bf16 workspace and run the library GEMM. The experts of a MoE block are
served together by the grouped kernel (csrc/int4_moe.hip) through an
Int4ExpertGroup.

The pinned dequantization, the exact expression and rounding of
models/loader._awq_dequant:

    w[n, k] = bf16_rne(float(q[n, k] - z[n, k // g]) * float(s[n, k // g]))

in fp32. `Int4Weight.dequant()` is the torch reference; both kernels
reproduce it bit for bit.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from kubeai_amd import ops

GROUPS = (32, 64, 128)
_CHUNK = 128  # k per packed chunk (4 lanes x 32 codes), see int4_gemm.hip


class Int4Weight:
    """One linear's quantized weight, logical [N, K].

    Physical packing (private to this class and csrc/int4_gemm.hip; built
    once, here). N is cut into tiles of 16 rows, K into chunks of 128 with
    the last chunk zero-padded:

      qp int32 [N/16, Kc, 64, 4]  unit kq*16 + nl holds the 32 consecutive-k
                                  codes of row tile*16 + nl from
                                  k = chunk*128 + kq*32; code j in word j//8,
                                  bits 4*(j%8)..+3 (one 16-byte lane load)
      sp fp16  [N/16, G, 16]      scales of the tile's 16 rows, per group
      zp uint8 [N/16, G, 8]       zero points, row nl in byte nl//2,
                                  bits 4*(nl%2)..+3

    All three are tile-major, so concatenation along N is a plain cat.
    """

    def __init__(self, qp, sp, zp, N: int, K: int, group: int):
        self.qp, self.sp, self.zp = qp, sp, zp
        self.N, self.K, self.group = int(N), int(K), int(group)
        if qp.is_cuda:
            # the large-M route dequantizes into a process-wide workspace;
            # sized here, when the weight is built, never at call time
            ops.int4_reserve_workspace(qp.device, self.N * self.K)

    # ---------------------------------------------------------------- build
    @staticmethod
    def check_shape(N: int, K: int, group: int) -> None:
        if group not in GROUPS:
            raise ValueError(f"int4: group size {group} not in {GROUPS}")
        if N % 16 or K % 32 or K % group:
            raise ValueError(
                f"int4: weight [{N}, {K}] with group {group} needs "
                "N % 16 == 0, K % 32 == 0 and K % group == 0"
            )

    @classmethod
    def from_codes(cls, q: torch.Tensor, z: torch.Tensor, s: torch.Tensor):
        """q uint8 [N, K] codes, z uint8 [N, K/g] zero points (both 0..15),
        s fp16 [N, K/g] scales."""
        N, K = q.shape
        if z.shape != s.shape or z.shape[0] != N or z.shape[1] == 0 or K % z.shape[1]:
            raise ValueError(
                f"int4: codes {tuple(q.shape)}, zeros {tuple(z.shape)}, "
                f"scales {tuple(s.shape)} do not describe one weight"
            )
        G = z.shape[1]
        group = K // G
        cls.check_shape(N, K, group)
        kc = (K + _CHUNK - 1) // _CHUNK
        qq = torch.zeros((N, kc * _CHUNK), dtype=torch.int64, device=q.device)
        qq[:, :K] = q.to(torch.int64) & 0xF
        # [tile, nl, chunk, kq, word, nib] -> [tile, chunk, kq, nl, word, nib]
        qq = qq.view(N // 16, 16, kc, 4, 4, 8).permute(0, 2, 3, 1, 4, 5)
        shifts = torch.arange(0, 32, 4, dtype=torch.int64, device=q.device)
        words = (qq << shifts).sum(-1)  # disjoint nibbles: sum == or
        words = torch.where(words >= 2**31, words - 2**32, words)
        qp = words.to(torch.int32).reshape(N // 16, kc, 64, 4).contiguous()
        sp = (
            s.to(torch.float16).view(N // 16, 16, G).permute(0, 2, 1).contiguous()
        )
        zz = (z.to(torch.uint8) & 0xF).view(N // 16, 16, G).permute(0, 2, 1)
        zz = zz.reshape(N // 16, G, 8, 2)
        zp = (zz[..., 0] | (zz[..., 1] << 4)).contiguous()
        return cls(qp, sp, zp, N, K, group)

    @classmethod
    def from_awq(cls, qweight, qzeros, scales):
        """AutoAWQ "gemm" tensors: qweight int32 [K, N/8], qzeros int32
        [K/g, N/8], scales fp16 [K/g, N]."""
        from kubeai_amd.models.loader import _awq_unpack

        q = _awq_unpack(qweight).t()  # [N, K]
        z = _awq_unpack(qzeros).t()   # [N, K/g]
        return cls.from_codes(
            q.to(torch.uint8), z.to(torch.uint8), scales.t().to(torch.float16)
        )

    @classmethod
    def quantize_rtn(cls, weight: torch.Tensor, group: int = 128):
        """Round-to-nearest min/max quantization per (row, group)."""
        N, K = weight.shape
        cls.check_shape(N, K, group)
        wg = weight.detach().float().view(N, K // group, group)
        mn = wg.min(dim=2).values
        mx = wg.max(dim=2).values
        scale = torch.clamp((mx - mn) / 15.0, min=1e-8)
        zero = torch.round(-mn / scale).clamp(0, 15)
        q = torch.round(wg / scale.unsqueeze(2) + zero.unsqueeze(2)).clamp(0, 15)
        return cls.from_codes(
            q.view(N, K).to(torch.uint8), zero.to(torch.uint8), scale.half()
        )

    @classmethod
    def cat(cls, weights: list["Int4Weight"]):
        """Concatenate along N (fused qkv, gate_up)."""
        w0 = weights[0]
        for w in weights[1:]:
            if (w.K, w.group) != (w0.K, w0.group):
                raise ValueError(
                    f"int4: cannot join [{w.N}, {w.K}] g={w.group} with "
                    f"[{w0.N}, {w0.K}] g={w0.group}"
                )
        return cls(
            torch.cat([w.qp for w in weights]),
            torch.cat([w.sp for w in weights]),
            torch.cat([w.zp for w in weights]),
            sum(w.N for w in weights), w0.K, w0.group,
        )

    # ----------------------------------------------------------------- read
    def codes(self):
        """(q [N, K], z [N, K/g], s [N, K/g]) back in logical order."""
        N, K = self.N, self.K
        G = K // self.group
        kc = self.qp.shape[1]
        dev = self.qp.device
        shifts = torch.arange(0, 32, 4, dtype=torch.int32, device=dev)
        nib = (self.qp.view(N // 16, kc, 4, 16, 4, 1) >> shifts) & 0xF
        q = nib.permute(0, 3, 1, 2, 4, 5).reshape(N, kc * _CHUNK)[:, :K]
        zz = torch.stack([self.zp & 0xF, self.zp >> 4], dim=-1)  # [N/16, G, 8, 2]
        z = zz.reshape(N // 16, G, 16).permute(0, 2, 1).reshape(N, G)
        s = self.sp.permute(0, 2, 1).reshape(N, G)
        return q, z, s

    def dequant(self) -> torch.Tensor:
        """bf16 [N, K], pure torch, any device: the reference."""
        q, z, s = self.codes()
        g = self.group
        zf = z.float().repeat_interleave(g, dim=1)
        sf = s.float().repeat_interleave(g, dim=1)
        return ((q.float() - zf) * sf).to(torch.bfloat16)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.qp, self.sp, self.zp))

    @property
    def device(self):
        return self.qp.device

    def to(self, device) -> "Int4Weight":
        return Int4Weight(
            self.qp.to(device), self.sp.to(device), self.zp.to(device),
            self.N, self.K, self.group,
        )


class Int4Linear(nn.Module):
    """Drop-in replacement for nn.Linear over an Int4Weight. It has no
    forward_quantized: the fp8-fused and MoE fp8 checks must not take it
    for an Fp8Linear."""

    def __init__(self, w: Int4Weight, bias: torch.Tensor | None = None):
        super().__init__()
        self.register_buffer("qweight", w.qp)
        self.register_buffer("scales", w.sp)
        self.register_buffer("qzeros", w.zp)
        self.out_features, self.in_features, self.group = w.N, w.K, w.group
        # the bias Parameter object is kept as it is (a checkpoint load may
        # still fill it in place)
        self.bias = bias

    def _apply(self, fn, *args, **kwargs):
        # .to()/.cuda(): re-wrap the moved buffers now, so the workspace is
        # reserved at the move, not at the first forward
        super()._apply(fn, *args, **kwargs)
        self._w = None
        self.int4
        return self

    @property
    def int4(self) -> Int4Weight:
        w = getattr(self, "_w", None)
        if w is None or w.qp is not self.qweight:
            w = self._w = Int4Weight(
                self.qweight, self.scales, self.qzeros,
                self.out_features, self.in_features, self.group,
            )
        return w

    @property
    def weight(self) -> torch.Tensor:
        """Dequantized bf16 for code paths that read .weight (LoRA base,
        tests)."""
        return self.int4.dequant()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = ops.int4_linear(x, self.int4)
        if self.bias is not None:
            y = y + self.bias
        return y


class Int4ExpertGroup:
    """The E Int4Weights of one MoE projection (every expert's gate_up_proj,
    or every expert's down_proj) as the grouped kernel takes them: the
    weights themselves, not a copy, and `table`, an int64 [E, 3] tensor on
    their device holding each expert's (qp, sp, zp) address.

    All experts share N, K, group size and device. The table is built here,
    when the experts are converted or moved; ops.int4_moe_linear only reads
    it (that call can run under graph capture, where building it would be a
    host-to-device copy inside the capture)."""

    def __init__(self, weights: list[Int4Weight]):
        if not weights:
            raise ValueError("int4 expert group: no experts")
        w0 = weights[0]
        for e, w in enumerate(weights):
            if (w.N, w.K, w.group) != (w0.N, w0.K, w0.group):
                raise ValueError(
                    f"int4 expert group: expert {e} is [{w.N}, {w.K}] "
                    f"g={w.group}, expert 0 is [{w0.N}, {w0.K}] g={w0.group}"
                )
            if w.device != w0.device:
                raise ValueError(
                    f"int4 expert group: expert {e} is on {w.device}, "
                    f"expert 0 on {w0.device}"
                )
            if not (w.qp.is_contiguous() and w.sp.is_contiguous()
                    and w.zp.is_contiguous()) or w.qp.data_ptr() % 16:
                raise ValueError(
                    f"int4 expert group: expert {e}'s packed tensors must be "
                    "contiguous and its codes 16-byte aligned"
                )
        self.weights = list(weights)
        self.E = len(weights)
        self.N, self.K, self.group = w0.N, w0.K, w0.group
        self.table = torch.tensor(
            [[w.qp.data_ptr(), w.sp.data_ptr(), w.zp.data_ptr()]
             for w in weights],
            dtype=torch.int64,
        ).to(w0.device)

    @property
    def device(self):
        return self.weights[0].device

    def table_on(self, device) -> torch.Tensor:
        if self.table.device != device:
            raise RuntimeError(
                f"int4 expert group lives on {self.table.device}, the call "
                f"is on {device}"
            )
        return self.table

    def holds(self, linears) -> bool:
        """Whether the group still describes exactly these Int4Linears'
        buffers (a buffer that was replaced leaves the table stale)."""
        return len(linears) == self.E and all(
            w.qp is lin.qweight and w.sp is lin.scales and w.zp is lin.qzeros
            for w, lin in zip(self.weights, linears)
        )


def expert_groups(experts):
    """(gate_up group, down group) of a list of expert MLPs when every
    projection is a bias-free Int4Linear, else None."""
    gate_up = [getattr(ex, "gate_up_proj", None) for ex in experts]
    down = [getattr(ex, "down_proj", None) for ex in experts]
    for lin in gate_up + down:
        if not isinstance(lin, Int4Linear) or lin.bias is not None:
            return None
    return (
        Int4ExpertGroup([lin.int4 for lin in gate_up]),
        Int4ExpertGroup([lin.int4 for lin in down]),
    )


# lm_head stays bf16, as in AWQ checkpoints
_TARGETS = ("qkv_proj", "o_proj", "gate_up_proj", "down_proj")


def convert_to_int4(model: nn.Module, group: int = 128) -> int:
    """Swap target nn.Linear modules (dense and MoE-expert alike) for
    Int4Linear, round-to-nearest; returns the count. Each bf16 parameter is
    released as soon as its replacement is installed."""
    n = 0
    for mod_name, mod in model.named_modules():
        for name in _TARGETS:
            child = getattr(mod, name, None)
            if not isinstance(child, nn.Linear):
                continue
            try:
                w = Int4Weight.quantize_rtn(child.weight, group)
            except ValueError as e:
                raise ValueError(f"{mod_name}.{name}: {e}") from None
            setattr(mod, name, Int4Linear(w, child.bias))
            n += 1
    # MoE blocks: the grouped kernel's address tables, built now that every
    # expert is in place
    for mod in model.modules():
        refresh = getattr(mod, "refresh_int4_groups", None)
        if refresh is not None:
            refresh()
    return n
