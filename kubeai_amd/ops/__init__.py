"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (deliberate, see repo instructions): on a ROCm GPU the HIP extension is
MANDATORY — if ``kubeai_amd._C`` failed to import, GPU-tensor calls raise
instead of silently falling back to eager PyTorch.  CPU tensors always use the
reference implementations (ref.py) so the engine logic is testable anywhere.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import torch

from . import ref

_C = None
_C_IMPORT_ERROR: Exception | None = None
try:  # built in-tree by `python setup.py build_ext --inplace` / __graft_entry__.build()
    from kubeai_amd import _C  # type: ignore[attr-defined,no-redef]
except Exception as e:  # pragma: no cover - exercised only when ext missing
    _C_IMPORT_ERROR = e


def have_hip_ext() -> bool:
    return _C is not None


def _require_ext() -> None:
    if _C is None:
        raise RuntimeError(
            "kubeai_amd HIP extension (kubeai_amd._C) is not built but a GPU "
            "tensor reached the ops layer. Build it with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Original import error: {_C_IMPORT_ERROR!r}"
        )


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        _require_ext()
        out = torch.empty_like(x)
        _C.rmsnorm(out, x, weight, eps)
        return out
    return ref.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(x, residual, weight, eps: float):
    """In-place on GPU: x <- rmsnorm(x + residual), residual <- x + residual."""
    if x.is_cuda:
        _require_ext()
        _C.fused_add_rmsnorm(x, residual, weight, eps)
        return x, residual
    return ref.fused_add_rmsnorm(x, residual, weight, eps)


def rope(q, k, positions, cos_sin):
    """In-place on GPU; returns (q, k)."""
    if q.is_cuda:
        _require_ext()
        _C.rope(q, k, positions, cos_sin)
        return q, k
    return ref.rope(q, k, positions, cos_sin)


def reshape_and_cache(k, v, k_cache, v_cache, slot_mapping) -> None:
    if k.is_cuda:
        _require_ext()
        _C.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
        return
    ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


def rope_and_cache(q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping):
    """rope(q, k) followed by reshape_and_cache(k, v, ...) in one launch.
    In-place on q and k on GPU; returns (q, k). q, k and v may each carry
    their own row stride (views into the fused qkv output, or separately
    contiguous tensors). Tokens with slot -1 are rotated but not cached."""
    if q.is_cuda:
        _require_ext()
        _C.rope_and_cache(
            q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping
        )
        return q, k
    q, k = ref.rope(q, k, positions, cos_sin)
    ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)
    return q, k


def paged_attention_decode(
    q, k_cache, v_cache, block_tables, seq_lens, scale: float, out=None,
    window: int = 0, softcap: float = 0.0, fp8_out: bool = False,
):
    """q may be a row-strided view (fused qkv output); out must be
    contiguous (allocated here if not supplied). window > 0 enables
    sliding-window attention (Mistral/Gemma2 style: keys in
    (pos-window, pos]).

    fp8_out=True returns (out, fp8, row_scale) where (fp8, row_scale) is
    quant_fp8(out.view(B, -1)): on GPU the flash-decoding merge step emits
    it directly (no separate quantization launch)."""
    if q.is_cuda:
        _require_ext()
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        if fp8_out:
            B = q.shape[0]
            o8 = torch.empty(
                (B, q.shape[1] * q.shape[2]), dtype=torch.float8_e4m3fn,
                device=q.device,
            )
            oscale = torch.empty(B, dtype=torch.float32, device=q.device)
            _C.paged_attention_decode_fp8(
                out, o8, oscale, q, k_cache, v_cache, block_tables, seq_lens,
                scale, window, softcap
            )
            return out, o8, oscale
        _C.paged_attention_decode(
            out, q, k_cache, v_cache, block_tables, seq_lens, scale, window,
            softcap
        )
        return out
    res = ref.paged_attention_decode(
        q, k_cache, v_cache, block_tables, seq_lens, scale, window=window,
        softcap=softcap,
    )
    if out is not None:
        out.copy_(res)
        res = out
    if fp8_out:
        o8, oscale = ref.quant_fp8(res.reshape(res.shape[0], -1))
        return res, o8, oscale
    return res


def decode_rope_fused() -> bool:
    """KUBEAI_DECODE_ROPE_FUSED=0 makes rope_cache_attention_decode run the
    two-launch sequence (rope_and_cache, then paged_attention_decode) on GPU.
    Read at call time: the equivalence tests and A/B runs flip it."""
    return os.environ.get("KUBEAI_DECODE_ROPE_FUSED", "1") != "0"


def rope_cache_attention_decode(
    q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping,
    block_tables, seq_lens, scale: float, out=None, window: int = 0,
    softcap: float = 0.0, fp8_out: bool = False,
):
    """A pure-decode step's rope_and_cache(...) followed by
    paged_attention_decode(..., fp8_out=...) in one call: same return value,
    and the same bytes in `out`, the fp8 output, the row scales and both
    caches.

    On GPU the decode kernel rotates q and k itself and writes the new K/V
    rows, so there is no rope launch. Unlike rope_and_cache it does NOT write
    the rotated q/k back: q, k and v are left untouched (nothing after
    attention reads them on a pure-decode step).

    Every row must be a decode row: slot_mapping[b] is row (L-1) % 16 of
    block block_tables[b][(L-1) // 16] with L = seq_lens[b], or negative
    (graph pad row: nothing is cached, the row attends what the cache
    holds). q, k and v keep independent row strides."""
    if q.is_cuda and decode_rope_fused():
        _require_ext()
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        o8 = oscale = None
        if fp8_out:
            o8, oscale = _empty_fp8_rows(
                (q.shape[0], q.shape[1] * q.shape[2]), q.device
            )
        _C.rope_cache_attention_decode(
            out, o8, oscale, q, k, v, positions, cos_sin, k_cache, v_cache,
            slot_mapping, block_tables, seq_lens, scale, window, softcap
        )
        return (out, o8, oscale) if fp8_out else out
    if not q.is_cuda:
        # the composition of the refs (out of place, q and k untouched)
        res = ref.rope_cache_attention_decode(
            q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping,
            block_tables, seq_lens, scale, window=window, softcap=softcap,
        )
        if out is not None:
            out.copy_(res)
            res = out
        if fp8_out:
            o8, oscale = ref.quant_fp8(res.reshape(res.shape[0], -1))
            return res, o8, oscale
        return res
    # GPU with the switch off: exactly the two launches, so q and k ARE
    # rotated in place here, as rope_and_cache does
    qr, _ = rope_and_cache(
        q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping
    )
    return paged_attention_decode(
        qr, k_cache, v_cache, block_tables, seq_lens, scale, out=out,
        window=window, softcap=softcap, fp8_out=fp8_out,
    )


def paged_attention_prefill(
    q, k_cache, v_cache, block_tables, query_start_loc, seq_lens, scale: float,
    out=None, window: int = 0, softcap: float = 0.0,
):
    if q.is_cuda:
        _require_ext()
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _C.paged_attention_prefill(
            out, q, k_cache, v_cache, block_tables, query_start_loc, seq_lens,
            scale, window, softcap
        )
        return out
    res = ref.paged_attention_prefill(
        q, k_cache, v_cache, block_tables, query_start_loc, seq_lens, scale,
        window=window, softcap=softcap,
    )
    if out is not None:
        out.copy_(res)
        return out
    return res


def silu_and_mul(x):
    if x.is_cuda:
        _require_ext()
        T, two_i = x.shape
        out = torch.empty((T, two_i // 2), dtype=x.dtype, device=x.device)
        _C.silu_and_mul(out, x)
        return out
    return ref.silu_and_mul(x)


def gelu_and_mul(x):
    """GeGLU (gemma family): gelu_tanh(gate) * up over packed [T, 2I]."""
    if x.is_cuda:
        _require_ext()
        T, two_i = x.shape
        out = torch.empty((T, two_i // 2), dtype=x.dtype, device=x.device)
        _C.gelu_and_mul(out, x)
        return out
    return ref.gelu_and_mul(x)


_USE_SKINNY = os.environ.get("KUBEAI_SKINNY_GEMM", "0") == "1"


def linear(x, weight):
    """GEMM dispatch. The hand-written weight-streaming kernel (skinny_gemm)
    currently loses to hipBLASLt on MI355X (direct 16 B row gathers do not
    coalesce; measured 0.3-0.65x — profiles/r01_results.md), so it is
    opt-in via KUBEAI_SKINNY_GEMM=1 until the LDS-staged variant lands."""
    if (
        _USE_SKINNY
        and x.is_cuda
        and x.dtype == torch.bfloat16
        and x.dim() == 2
        and 1 <= x.shape[0] <= 64
        and weight.shape[1] % 64 == 0
        and weight.shape[0] % 64 == 0
        and x.is_contiguous()
        and weight.is_contiguous()
    ):
        _require_ext()
        y = torch.empty(
            (x.shape[0], weight.shape[0]), dtype=x.dtype, device=x.device
        )
        _C.skinny_gemm(y, x, weight)
        return y
    return torch.nn.functional.linear(x, weight)


# ---------------- int4 (W4A16) ----------------
# `w` below is an engine.quant_int4.Int4Weight (packed qp/sp/zp + N, K, group).

# Largest M the fused dequant-GEMM kernel takes; above it int4_linear runs
# int4_dequant + the library GEMM. See docs/kernels.md for how it is set.
INT4_M_FUSED = int(os.environ.get("KUBEAI_INT4_M_FUSED", "64"))

# device -> flat bf16 buffer the large-M route dequantizes into. Grown only by
# int4_reserve_workspace, which every GPU Int4Weight calls at construction:
# that route can run under graph capture and must not allocate there.
_INT4_WORKSPACE: dict = {}


def int4_reserve_workspace(device, numel: int) -> None:
    device = torch.device(device)
    ws = _INT4_WORKSPACE.get(device)
    if ws is None or ws.numel() < numel:
        _INT4_WORKSPACE[device] = torch.empty(
            numel, dtype=torch.bfloat16, device=device
        )


def int4_dequant(w, out=None):
    """Packed int4 weight -> bf16 [N, K], bit-identical to w.dequant()."""
    if not w.qp.is_cuda:
        res = w.dequant()
        if out is not None:
            out.copy_(res)
            return out
        return res
    _require_ext()
    if out is None:
        out = torch.empty((w.N, w.K), dtype=torch.bfloat16, device=w.qp.device)
    _C.int4_dequant(out, w.qp, w.sp, w.zp, w.N, w.K, w.group)
    return out


def int4_linear(x, w):
    """y[M, N] = x[M, K] @ w.dequant()^T, bf16, fp32 accumulation. x may be a
    row-strided view with a contiguous last dimension."""
    if not x.is_cuda:
        return torch.nn.functional.linear(x, w.dequant())
    _require_ext()
    if x.dim() != 2:
        return int4_linear(x.reshape(-1, x.shape[-1]), w).view(*x.shape[:-1], w.N)
    M = x.shape[0]
    if 1 <= M <= min(INT4_M_FUSED, 64):
        if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
            x = x.contiguous()
        y = torch.empty((M, w.N), dtype=torch.bfloat16, device=x.device)
        _C.int4_gemm(y, x, w.qp, w.sp, w.zp, w.N, w.K, w.group)
        return y
    ws = _INT4_WORKSPACE.get(x.device)
    if ws is None or ws.numel() < w.N * w.K:
        raise RuntimeError(
            "int4 workspace was not reserved for this weight "
            f"([{w.N}, {w.K}] on {x.device})"
        )
    dense = int4_dequant(w, out=ws[: w.N * w.K].view(w.N, w.K))
    return torch.nn.functional.linear(x, dense)


# ---------------- int4 MoE: grouped expert GEMMs, routed on the device ------
# `group` below is an engine.quant_int4.Int4ExpertGroup (the E Int4Weights of
# one projection and the device table of their addresses); `selected` is
# torch.topk's int64 [T, k].

# Largest T for which MoEMLP takes int4_moe_mlp; above it, and at 0, it keeps
# the dense expert loop. See docs/kernels.md for how it is set.
INT4_MOE_T = int(os.environ.get("KUBEAI_INT4_MOE_T", "64"))


def int4_moe_linear(x, selected, group, row_div: int, out=None):
    """y[t*k + j] = x[(t*k + j) // row_div] @ W[selected[t, j]]^T, bf16
    [T*k, N], one launch for all experts. row_div = k: the k pairs of a token
    share its row of x [T, K]; row_div = 1: x is [T*k, K]. Every row is
    bit-equal to int4_linear's for that row and expert. T <= 64."""
    if not x.is_cuda:
        res = ref.moe_linear(
            x, selected, [w.dequant() for w in group.weights], row_div
        )
        if out is not None:
            out.copy_(res)
            return out
        return res
    _require_ext()
    if x.dim() == 2 and (x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16):
        x = x.contiguous()
    if out is None:
        out = torch.empty(
            (selected.numel(), group.N), dtype=torch.bfloat16, device=x.device
        )
    _C.int4_moe_gemm(
        out, x, selected, group.table_on(x.device), row_div, group.E, group.N,
        group.K, group.group,
    )
    return out


def moe_combine(y, selected, weights, n_experts: int | None = None):
    """out[t] = sum_j weights[t, j] * y[t*k + j] -> [T, H], added up as
    MoEMLP's dense loop does (ref.moe_combine). One launch on GPU."""
    if not y.is_cuda:
        return ref.moe_combine(y, selected, weights, n_experts)
    _require_ext()
    out = torch.empty(
        (selected.shape[0], y.shape[1]), dtype=y.dtype, device=y.device
    )
    _C.moe_combine(out, y, selected, weights, n_experts or 0)
    return out


def int4_moe_mlp(x, selected, weights, gate_up_group, down_group):
    """The SwiGLU MoE block over int4 experts: [T, H] -> [T, H], equal to
    MoEMLP's dense loop. Four launches on GPU (gate_up, silu_and_mul, down,
    combine), and only the routed experts' weights are read."""
    if not x.is_cuda:
        return ref.moe_mlp(
            x, selected, weights,
            [w.dequant() for w in gate_up_group.weights],
            [w.dequant() for w in down_group.weights],
        )
    h = int4_moe_linear(x, selected, gate_up_group, selected.shape[1])
    y = int4_moe_linear(silu_and_mul(h), selected, down_group, 1)
    return moe_combine(y, selected, weights, gate_up_group.E)


# ---------------- fp8 MoE: grouped expert GEMMs, routed on the device -------
# `group` below is an engine.quant.Fp8ExpertGroup (the E Fp8Linears of one
# projection and the device table of their addresses).


def fp8_moe_t() -> int:
    """Largest T for which MoEMLP takes fp8_moe_mlp: KUBEAI_FP8_MOE_T, 0 (the
    dense expert loop at every T) when unset, at most 64. The grouped path
    sums in another order than the dense loop's _scaled_mm, so it is opt-in
    (profiles/r11_fp8_moe.md). Read at call time: the tests and A/B runs flip
    it."""
    try:
        limit = int(os.environ.get("KUBEAI_FP8_MOE_T", "0"))
    except ValueError:
        return 0
    return max(0, min(limit, 64))


def fp8_moe_linear(xq, xs, selected, group, row_div: int, out=None):
    """y[t*k + j] = bf16((xq[r] @ wq_e^T) * xs[r] * ws_e) with r =
    (t*k + j) // row_div and e = selected[t, j]: bf16 [T*k, N], one launch for
    all experts. xq is e4m3 [R, K] with fp32 row scales xs [R]. row_div = k:
    the k pairs of a token share its row; row_div = 1: xq is [T*k, K]. Every
    row is Fp8Linear.forward_quantized's for that row and expert up to the
    order of the fp32 sum, and has the same bits whatever else is in the
    batch. T <= 64."""
    if not xq.is_cuda:
        res = ref.fp8_moe_linear(
            xq, xs, selected,
            [(lin.weight_fp8, lin.weight_scale) for lin in group.linears],
            row_div,
        )
        if out is not None:
            out.copy_(res)
            return out
        return res
    _require_ext()
    if xq.dim() == 2 and (
        xq.stride(1) != 1 or xq.stride(0) % 16 or xq.data_ptr() % 16
    ):
        xq = xq.contiguous()
    if out is None:
        out = torch.empty(
            (selected.numel(), group.N), dtype=torch.bfloat16, device=xq.device
        )
    _C.fp8_moe_gemm(
        out, xq, xs.reshape(-1), selected, group.table_on(xq.device), row_div,
        group.E, group.N, group.K,
    )
    return out


def fp8_moe_mlp(x, selected, weights, gate_up_group, down_group):
    """The SwiGLU MoE block over fp8 experts: [T, H] -> [T, H]. The dense
    loop's operations on the routed pairs only: quant_fp8, gate_up,
    silu_and_mul_fp8, down, combine. Five launches on GPU, and only the
    routed experts' weights are read."""
    xq, xs = quant_fp8(x)
    h = fp8_moe_linear(xq, xs, selected, gate_up_group, selected.shape[1])
    a8, a_scale = silu_and_mul_fp8(h)
    y = fp8_moe_linear(a8, a_scale, selected, down_group, 1)
    return moe_combine(y, selected, weights, gate_up_group.E)


def _empty_fp8_rows(shape, device):
    """Uninitialised (e4m3 `shape`, f32 [shape[0]] row scales) for an fp8
    producer to fill."""
    out = torch.empty(shape, dtype=torch.float8_e4m3fn, device=device)
    scale = torch.empty(shape[0], dtype=torch.float32, device=device)
    return out, scale


def rmsnorm_fp8(x, weight, eps: float):
    """GPU-only: rmsnorm with fused per-row fp8 quantization."""
    _require_ext()
    out, scale = _empty_fp8_rows(x.shape, x.device)
    _C.rmsnorm_fp8(out, scale, x, weight, eps)
    return out, scale


def fused_add_rmsnorm_fp8(x, residual, weight, eps: float):
    """GPU-only, in-place residual update; returns (fp8 out, row scales)."""
    _require_ext()
    out, scale = _empty_fp8_rows(x.shape, x.device)
    _C.fused_add_rmsnorm_fp8(out, scale, x, residual, weight, eps)
    return out, scale


def silu_and_mul_fp8(x):
    if not x.is_cuda:
        return ref.quant_fp8(ref.silu_and_mul(x))
    _require_ext()
    T, two_i = x.shape
    out, scale = _empty_fp8_rows((T, two_i // 2), x.device)
    _C.silu_and_mul_fp8(out, scale, x)
    return out, scale


def quant_fp8(x):
    if not x.is_cuda:
        return ref.quant_fp8(x)
    _require_ext()
    out, scale = _empty_fp8_rows(x.shape, x.device)
    _C.quant_fp8(out, scale, x)
    return out, scale


# longest row the row kernels take (row_kernels.hip::kMaxH)
_QUANT_DIV_MAX_H = 32768


def quant_fp8_div(x):
    """Row quantization in the division form Fp8Linear.forward pins
    (ref.quant_fp8_div): (e4m3 [T, H], fp32 scales [T, 1]). One launch for a
    2-D contiguous bf16 GPU tensor with H % 8 == 0, byte-equal to the torch
    chain, which serves every other input."""
    if (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and x.dim() == 2
        and x.is_contiguous()
        and x.shape[1] % 8 == 0
        and 0 < x.shape[1] <= _QUANT_DIV_MAX_H
        and os.environ.get("KUBEAI_QUANT_DIV_KERNEL", "1") != "0"
    ):
        _require_ext()
        out, scale = _empty_fp8_rows(x.shape, x.device)
        _C.quant_fp8_div(out, scale, x)
        return out, scale.view(-1, 1)
    return ref.quant_fp8_div(x)


def _row_kernel_ok(x) -> bool:
    """A [T, H] tensor the row kernels take as it is."""
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and x.dim() == 2
        and x.is_contiguous()
        and x.shape[1] % 8 == 0
        and 0 < x.shape[1] <= _QUANT_DIV_MAX_H
    )


def embed_rmsnorm_fp8(ids, table, weight, eps: float):
    """x = table[ids] followed by rmsnorm_fp8(x, weight, eps): returns
    (x, fp8 out, row scales), the three byte-equal to that sequence.

    One launch for int32 1-D contiguous ids and a contiguous bf16 table on
    GPU (the kernel reads row ids[t] itself and clamps the id into the
    table); the embedding lookup and rmsnorm_fp8 (on CPU: the reference
    norm and quantization) for every other input."""
    if (
        _row_kernel_ok(table)
        and ids.is_cuda
        and ids.dtype == torch.int32
        and ids.dim() == 1
        and ids.is_contiguous()
        and weight.dtype == torch.bfloat16
    ):
        _require_ext()
        T, H = ids.shape[0], table.shape[1]
        x = torch.empty((T, H), dtype=table.dtype, device=table.device)
        out, scale = _empty_fp8_rows((T, H), table.device)
        _C.embed_rmsnorm_fp8(out, scale, x, ids, table, weight, eps)
        return x, out, scale
    x = torch.nn.functional.embedding(ids.long(), table)
    if x.is_cuda:
        return (x, *rmsnorm_fp8(x, weight, eps))
    return (x, *ref.quant_fp8(ref.rmsnorm(x, weight, eps)))


def fused_add_rmsnorm_fp8_div(x, residual, weight, eps: float,
                              write_rows: bool = False):
    """quant_fp8_div(fused_add_rmsnorm(x, residual, weight, eps)[0]):
    (e4m3 [T, H], fp32 scales [T, 1]), byte-equal to the two ops.

    One launch for 2-D contiguous bf16 on GPU. With write_rows it also
    updates x and residual in place as fused_add_rmsnorm does; without it
    the kernel only reads them. Every other input runs the two ops (which on
    GPU update x and residual), so a caller that passes write_rows=False
    must not read either afterwards."""
    if (
        _row_kernel_ok(x)
        and residual.is_contiguous()
        and residual.shape == x.shape
        and residual.dtype == x.dtype
        and weight.dtype == torch.bfloat16
    ):
        _require_ext()
        out, scale = _empty_fp8_rows(x.shape, x.device)
        _C.fused_add_rmsnorm_fp8_div(
            out, scale, x, residual, weight, eps, write_rows
        )
        return out, scale.view(-1, 1)
    y, _ = fused_add_rmsnorm(x, residual, weight, eps)
    return quant_fp8_div(y)


def greedy_sample(logits):
    if logits.is_cuda:
        _require_ext()
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        _C.greedy_sample(out, logits)
        return out
    return ref.greedy_sample(logits)


def gumbel_sample(logits, temperature, seeds, step: int):
    if logits.is_cuda:
        _require_ext()
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        _C.gumbel_sample(out, logits, temperature, seeds, step)
        return out
    return ref.gumbel_sample(logits, temperature, seeds, step)


class SampleResult(NamedTuple):
    """What a *_sample_logprob op returns. On GPU the three tensors are views
    of `packed`, one int64 [2B] buffer (B tokens, then B fp32 logprobs and B
    fp32 lse), so a caller can bring tokens and logprobs to the host in one
    copy: `sample_to_host`."""

    tokens: torch.Tensor   # [B] int64
    logprob: torch.Tensor  # [B] fp32: logits[b, token] - lse[b]
    lse: torch.Tensor      # [B] fp32: logsumexp of row b
    packed: torch.Tensor | None = None


def _empty_sample_result(logits) -> SampleResult:
    B = logits.shape[0]
    packed = torch.empty(2 * B, dtype=torch.int64, device=logits.device)
    f = packed[B:].view(torch.float32)
    return SampleResult(packed[:B], f[:B], f[B:], packed)


def sample_to_host(res: SampleResult) -> tuple[list[int], list[float]]:
    """(tokens, logprobs) as Python lists: one device-to-host copy."""
    if res.packed is None or not res.packed.is_cuda:
        return res.tokens.tolist(), res.logprob.tolist()
    B = res.tokens.shape[0]
    host = res.packed[: B + (B + 1) // 2].cpu()
    return host[:B].tolist(), host[B:].view(torch.float32)[:B].tolist()


def greedy_sample_logprob(logits) -> SampleResult:
    """greedy_sample's token, plus its log-probability and the row's
    logsumexp. On GPU the sampler's own two launches produce all three."""
    if logits.is_cuda:
        _require_ext()
        res = _empty_sample_result(logits)
        _C.greedy_sample_logprob(res.tokens, res.logprob, res.lse, logits)
        return res
    return SampleResult(*ref.greedy_sample_logprob(logits))


def gumbel_sample_logprob(logits, temperature, seeds, step: int) -> SampleResult:
    """gumbel_sample's token, plus its log-probability and the row's
    logsumexp, both over `logits` as passed (untempered, no noise)."""
    if logits.is_cuda:
        _require_ext()
        res = _empty_sample_result(logits)
        _C.gumbel_sample_logprob(
            res.tokens, res.logprob, res.lse, logits, temperature, seeds, step
        )
        return res
    return SampleResult(
        *ref.gumbel_sample_logprob(logits, temperature, seeds, step)
    )


def token_logprobs(logits, tokens):
    """(logprob [B], lse [B]) of int64 tokens[b] in row b of fp32 logits, for
    tokens that do not come from a *_sample_logprob op. One launch on GPU;
    lse is bit-identical to the one those ops return. Like the samplers, the
    GPU kernel also takes bf16 logits, with the results of logits.float()."""
    if logits.is_cuda:
        _require_ext()
        B = logits.shape[0]
        out = torch.empty((2, B), dtype=torch.float32, device=logits.device)
        _C.token_logprobs(out[0], out[1], logits, tokens)
        return out[0], out[1]
    return ref.token_logprobs(logits, tokens)


def nucleus_stats(logits, temps):
    """Per-row (max, sum exp((x-max)/t)) for rejection nucleus sampling."""
    if logits.is_cuda:
        _require_ext()
        S = logits.shape[0]
        m = torch.empty(S, dtype=torch.float32, device=logits.device)
        z = torch.empty_like(m)
        _C.nucleus_stats(m, z, logits, temps)
        return m, z
    t = temps.clamp_min(1e-6).unsqueeze(1)
    m = logits.max(dim=-1).values
    z = torch.exp((logits - m.unsqueeze(1)) / t).sum(-1)
    return m, z


def nucleus_accept(logits, cand, m, z, temps, top_ps, top_ks):
    """uint8 mask: sampled token lies in the top-p/top-k nucleus
    (probability mass strictly above it < top_p, rank < top_k);
    greedy rows always accept."""
    if logits.is_cuda:
        _require_ext()
        ok = torch.empty(logits.shape[0], dtype=torch.uint8,
                         device=logits.device)
        _C.nucleus_accept(ok, logits, cand, m, z, temps, top_ps, top_ks)
        return ok
    t = temps.clamp_min(1e-6).unsqueeze(1)
    lt = logits.gather(1, cand.view(-1, 1))
    above = logits > lt
    mass = (torch.exp((logits - m.unsqueeze(1)) / t) * above).sum(-1) / z
    cnt = above.sum(-1)
    ok = (mass < top_ps) & ((top_ks <= 0) | (cnt < top_ks)) | (temps <= 0)
    return ok.to(torch.uint8)
