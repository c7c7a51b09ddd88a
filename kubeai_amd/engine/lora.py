"""LoRA adapter manager (multi-adapter serving, vLLM-style semantics).

Adapters target the attention projections (q/k/v/o). A mixed batch carries
per-token adapter ids (ForwardBatch.lora_ids); apply() computes

    y[tok] += B_a (A_a x[tok]) * (alpha / r)      for tok with adapter a

grouped per adapter — the segmented-gather form of SGMV. Decode-sized steps
on GPU (T <= ops.lora_batched_t()) serve all adapters of the batch in two
launches instead (ops.lora_apply, csrc/lora_batched.hip): every loaded
adapter owns a slot, ForwardBatch.lora_slots carries the rows' slots, and one
LoraTable per (target, layer) holds the slots' weight addresses on the device.
Nothing on that path depends on which adapters a batch names, so the decode
step is graph-captured with adapters loaded (runner.py). Weight format:
HF PEFT safetensors when `path` exists; otherwise deterministic random-init
(rank 16) for synthetic/benchmark use (no network for real checkpoints).

KV-cache isolation: the adapter id doubles as the BlockManager salt, so
prefix blocks are never shared across adapters (kvcache.py).
"""
from __future__ import annotations

import os
import struct
from typing import Optional

import torch

from kubeai_amd import ops


class LoraTable:
    """The adapters of one (target, layer) as ops.lora_apply takes them: `dev`,
    an int64 [slots, 4] device tensor of (A address, B address, R, scale as
    fp32 bits) per slot, `host`, its host copy (the launcher checks the rows
    there, without a sync), and `rows`, the (A, B, scale) the addresses point
    at. Slot 0 is "no adapter"; R == 0 is "nothing to add".

    `dev` is allocated once: set_row and clear_row rewrite it in place, in
    stream order, so a captured graph that reads it stays valid."""

    SLOTS = 16  # slot 0 plus 15 adapters: the slot dimension of both grids
    MAX_RANK = 64

    def __init__(self, K: int, N: int, device, slots: int = SLOTS):
        self.K, self.N = K, N
        self.host = torch.zeros(slots, 4, dtype=torch.int64)
        self.dev = torch.zeros(slots, 4, dtype=torch.int64, device=device)
        self.rows: list = [None] * slots

    def set_row(self, slot: int, A: torch.Tensor, B: torch.Tensor, scale: float):
        """A [R, K], B [N, R], bf16, contiguous, R % 8 == 0, R <= 64."""
        if not 1 <= slot < len(self.rows):
            raise RuntimeError(f"lora table: slot {slot} outside [1, {len(self.rows)})")
        if self.K % 8 or self.N % 16:
            raise RuntimeError(
                f"lora table: K {self.K} and N {self.N}, need multiples of 8 and 16"
            )
        R = A.shape[0]
        if R % 8 or not 0 < R <= self.MAX_RANK:
            raise RuntimeError(
                f"lora table: rank {R}, need a multiple of 8 up to {self.MAX_RANK}"
            )
        if tuple(A.shape) != (R, self.K) or tuple(B.shape) != (self.N, R):
            raise RuntimeError(
                f"lora table: A {list(A.shape)} and B {list(B.shape)}, need "
                f"[{R}, {self.K}] and [{self.N}, {R}]"
            )
        for w in (A, B):
            if (
                w.dtype != torch.bfloat16 or w.device != self.dev.device
                or not w.is_contiguous() or w.data_ptr() % 16
            ):
                raise RuntimeError(
                    "lora table: A and B must be contiguous bf16 on the "
                    "table's device, 16-byte aligned"
                )
        packed = struct.pack("<f", scale)
        self.host[slot] = torch.tensor(
            [A.data_ptr(), B.data_ptr(), R, struct.unpack("<I", packed)[0]],
            dtype=torch.int64,
        )
        self.dev[slot].copy_(self.host[slot])
        self.rows[slot] = (A, B, struct.unpack("<f", packed)[0])

    def clear_row(self, slot: int) -> None:
        """R = 0 on the device first; the tensors are released after it."""
        self.host[slot] = 0
        self.dev[slot].copy_(self.host[slot])
        self.rows[slot] = None


class LoRAManager:
    DEFAULT_RANK = 16
    TARGETS = ("qkv", "o", "gate_up", "down")

    def __init__(self, model, device, dtype):
        self.model = model
        self.device = device
        self.dtype = dtype
        # adapters[lora_id][target] = list over layers of (A [r,in], B [out,r], scale)
        self.adapters: dict[int, dict[str, list[tuple[torch.Tensor, torch.Tensor, float]]]] = {}
        # batched path: lora_id -> slot, the ids whose ranks it cannot take,
        # tables[target][layer] (built at the first load) and the K-split
        # workspace all applies share
        self.slots: dict[int, int] = {}
        self._unbatchable: set[int] = set()
        self.tables: dict[str, list[LoraTable]] | None = None
        self.vpart: torch.Tensor | None = None
        model.lora_manager = self
        for m in model.modules():
            if hasattr(m, "qkv_proj"):  # Attention modules
                object.__setattr__(m, "_lora_manager", self)
            # dense per-layer MLPs (layer_idx set); MoE expert MLPs excluded
            if hasattr(m, "gate_up_proj") and getattr(m, "layer_idx", None) is not None:
                object.__setattr__(m, "_lora_manager", self)

    # ------------------------------------------------------------------
    def load(self, lora_id: int, path: Optional[str]) -> None:
        if lora_id in self.adapters:
            return
        if path and os.path.isdir(path) and _peft_weights_present(path):
            self.adapters[lora_id] = self._load_peft(path)
        else:
            self.adapters[lora_id] = self._random_adapter(lora_id)
        self._assign_slot(lora_id)

    def unload(self, lora_id: int) -> None:
        slot = self.slots.pop(lora_id, None)
        if slot is not None:
            for tables in self.tables.values():
                for table in tables:
                    table.clear_row(slot)
        self._unbatchable.discard(lora_id)
        self.adapters.pop(lora_id, None)

    def slot_of(self, lora_id: int) -> Optional[int]:
        return self.slots.get(lora_id)

    def _assign_slot(self, lora_id: int) -> None:
        """The lowest free slot, and the adapter's rows in every table. An
        adapter stays without a slot when none is free or when one of its
        ranks is not a multiple of 8 up to 64: steps then keep the sgmv loop."""
        adapter = self.adapters[lora_id]
        if self.tables is None:
            self.tables = {
                tgt: [
                    LoraTable(A.shape[1], B.shape[0], self.device)
                    for A, B, _ in layers
                ]
                for tgt, layers in adapter.items()
            }
            if torch.device(self.device).type == "cuda":
                self.vpart = ops.lora_vpart(self.device)
        # placeholders of missing targets (scale 0) are R = 0 rows
        live = [
            (tgt, layer, row)
            for tgt, layers in adapter.items()
            for layer, row in enumerate(layers)
            if row[2] != 0.0
        ]
        free = set(range(1, LoraTable.SLOTS)) - set(self.slots.values())
        if not free:
            return
        slot = min(free)
        try:
            for tgt, layer, (A, B, scale) in live:
                self.tables[tgt][layer].set_row(slot, A, B, scale)
        except RuntimeError:  # a rank or layout the batched kernels do not take
            for tables in self.tables.values():
                for table in tables:
                    table.clear_row(slot)
            self._unbatchable.add(lora_id)
            return
        self.slots[lora_id] = slot

    def batched(self, T: int, on_gpu: bool) -> bool:
        """Whether apply serves a step of T rows with ops.lora_apply."""
        return (
            on_gpu
            and 1 <= T <= ops.lora_batched_t()
            and not self._unbatchable
            and len(self.slots) == len(self.adapters)
        )

    @property
    def active(self) -> bool:
        return bool(self.adapters)

    # ------------------------------------------------------------------
    def _random_adapter(self, lora_id: int):
        g = torch.Generator(device="cpu").manual_seed(lora_id)
        r = self.DEFAULT_RANK
        cfg = self.model.cfg
        H = cfg.hidden_size
        qkv_out = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
        o_in = cfg.num_attention_heads * cfg.head_dim
        I = cfg.intermediate_size
        moe = cfg.num_local_experts > 0  # MoE: adapters stay attention-only
        out = {t: [] for t in self.TARGETS}
        for _ in range(cfg.num_hidden_layers):
            shapes = [("qkv", (H, qkv_out)), ("o", (o_in, H))]
            if not moe:
                shapes += [("gate_up", (H, 2 * I)), ("down", (I, H))]
            for tgt, (din, dout) in shapes:
                A = (torch.randn(r, din, generator=g) * 0.05).to(self.device, self.dtype)
                B = (torch.randn(dout, r, generator=g) * 0.5).to(self.device, self.dtype)
                out[tgt].append((A, B, 2.0 / r))
        return out

    def _load_peft(self, path: str):
        from safetensors.torch import load_file
        import json

        alpha, r = 16.0, self.DEFAULT_RANK
        cfg_path = os.path.join(path, "adapter_config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as f:
                acfg = json.load(f)
            alpha = float(acfg.get("lora_alpha", 16))
            r = int(acfg.get("r", 16))
        weights = load_file(_peft_weights_present(path))
        cfg = self.model.cfg
        out = {t: [] for t in self.TARGETS}
        for layer in range(cfg.num_hidden_layers):
            # fuse q/k/v adapters into the qkv slot (block-diagonal A, stacked B)
            parts = []
            for proj in ("q_proj", "k_proj", "v_proj"):
                key = _find_key(weights, layer, proj)
                parts.append(key)
            As, Bs = [], []
            for key in parts:
                if key is None:
                    As.append(None)
                    Bs.append(None)
                else:
                    As.append(weights[key + ".lora_A.weight"])
                    Bs.append(weights[key + ".lora_B.weight"])
            H = cfg.hidden_size
            q_out = cfg.num_attention_heads * cfg.head_dim
            kv_out = cfg.num_key_value_heads * cfg.head_dim
            outs = (q_out, kv_out, kv_out)
            n = sum(1 for a in As if a is not None)
            if n == 0:
                A = torch.zeros(1, H)
                B = torch.zeros(q_out + 2 * kv_out, 1)
            else:
                A = torch.cat([a for a in As if a is not None], dim=0)  # [n*r, H]
                B = torch.zeros(q_out + 2 * kv_out, A.shape[0])
                row, col = 0, 0
                for a, b, dout in zip(As, Bs, outs):
                    if a is not None:
                        B[row : row + dout, col : col + a.shape[0]] = b
                        col += a.shape[0]
                    row += dout
            out["qkv"].append(
                (A.to(self.device, self.dtype), B.to(self.device, self.dtype), alpha / r)
            )
            okey = _find_key(weights, layer, "o_proj")
            if okey is None:
                out["o"].append(
                    (
                        torch.zeros(1, q_out, device=self.device, dtype=self.dtype),
                        torch.zeros(H, 1, device=self.device, dtype=self.dtype),
                        0.0,
                    )
                )
            else:
                out["o"].append(
                    (
                        weights[okey + ".lora_A.weight"].to(self.device, self.dtype),
                        weights[okey + ".lora_B.weight"].to(self.device, self.dtype),
                        alpha / r,
                    )
                )
            # MLP targets: gate+up fused block-diagonally, down direct
            I = cfg.intermediate_size
            gkey = _find_key(weights, layer, "gate_proj", "mlp")
            ukey = _find_key(weights, layer, "up_proj", "mlp")
            if gkey is None and ukey is None:
                out["gate_up"].append(
                    (torch.zeros(1, H, device=self.device, dtype=self.dtype),
                     torch.zeros(2 * I, 1, device=self.device, dtype=self.dtype),
                     0.0)
                )
            else:
                As2, Bs2 = [], []
                for key, row in ((gkey, 0), (ukey, I)):
                    if key is not None:
                        As2.append((weights[key + ".lora_A.weight"], row))
                        Bs2.append(weights[key + ".lora_B.weight"])
                A2 = torch.cat([a for a, _ in As2], dim=0)  # [n*r, H]
                B2 = torch.zeros(2 * I, A2.shape[0])
                col = 0
                for (a, row), bmat in zip(As2, Bs2):
                    B2[row : row + I, col : col + a.shape[0]] = bmat
                    col += a.shape[0]
                out["gate_up"].append(
                    (A2.to(self.device, self.dtype),
                     B2.to(self.device, self.dtype), alpha / r)
                )
            dkey = _find_key(weights, layer, "down_proj", "mlp")
            if dkey is None:
                out["down"].append(
                    (torch.zeros(1, I, device=self.device, dtype=self.dtype),
                     torch.zeros(H, 1, device=self.device, dtype=self.dtype),
                     0.0)
                )
            else:
                out["down"].append(
                    (weights[dkey + ".lora_A.weight"].to(self.device, self.dtype),
                     weights[dkey + ".lora_B.weight"].to(self.device, self.dtype),
                     alpha / r)
                )
        return out

    # ------------------------------------------------------------------
    def apply(
        self,
        layer_idx: int,
        target: str,
        x: torch.Tensor,  # [T, in]
        y: torch.Tensor,  # [T, out] += delta (in-place)
        lora_ids: torch.Tensor,  # [T] int32
        lora_slots: Optional[torch.Tensor] = None,  # [T] int32
    ) -> None:
        """Decode-sized steps on GPU: ops.lora_apply over the rows' slots, two
        launches for all adapters and no sync. Otherwise the segmented LoRA
        matmul: per-adapter token groups; one hand-written SGMV kernel launch
        per adapter on GPU (csrc/sgmv.hip)."""
        if lora_slots is not None and self.batched(x.shape[0], x.is_cuda):
            ops.lora_apply(
                y, x, lora_slots, self.tables[target][layer_idx], self.vpart
            )
            return
        present = torch.unique(lora_ids)
        for lid_t in present:
            lid = int(lid_t)
            if lid == 0 or lid not in self.adapters:
                continue
            A, B, s = self.adapters[lid][target][layer_idx]
            idx = (lora_ids == lid_t).nonzero(as_tuple=True)[0]
            if x.is_cuda:
                from kubeai_amd import _C

                _C.sgmv(y, x, A, B, idx, s)
            else:
                xs = x[idx]
                y[idx] += (xs @ A.T @ B.T) * s


def _peft_weights_present(path: str) -> Optional[str]:
    for f in ("adapter_model.safetensors", "model.safetensors"):
        p = os.path.join(path, f)
        if os.path.exists(p):
            return p
    return None


def _find_key(
    weights: dict, layer: int, proj: str, sub: str = "self_attn"
) -> Optional[str]:
    for prefix in (
        f"base_model.model.model.layers.{layer}.{sub}.{proj}",
        f"model.layers.{layer}.{sub}.{proj}",
    ):
        if prefix + ".lora_A.weight" in weights:
            return prefix
    return None
