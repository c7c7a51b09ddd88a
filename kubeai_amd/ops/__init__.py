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
    # head_dim 64 has no rope-in-kernel form: its decode kernel
    # (attention_decode_hd64.hip) takes rotated q, so the two launches run
    if q.is_cuda and decode_rope_fused() and q.shape[-1] != 64:
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
    # GPU with the switch off, or head_dim 64: exactly the two launches, so q
    # and k ARE rotated in place here, as rope_and_cache does
    qr, _ = rope_and_cache(
        q, k, v, positions, cos_sin, k_cache, v_cache, slot_mapping
    )
    return paged_attention_decode(
        qr, k_cache, v_cache, block_tables, seq_lens, scale, out=out,
        window=window, softcap=softcap, fp8_out=fp8_out,
    )


def append_attn() -> bool:
    """KUBEAI_APPEND_ATTN=1 lets paged_attention_prefill hand the shapes
    _C.append_plan takes (a short chunk over a long cached context) to
    paged_attention_append. Off by default: it moves low bits of prefill
    outputs. Read at call time: the routing test and A/B runs flip it."""
    return os.environ.get("KUBEAI_APPEND_ATTN", "0") == "1"


def paged_attention_append(
    q, k_cache, v_cache, block_tables, query_start_loc, seq_lens, scale: float,
    out=None, n_splits: int = 0, window: int = 0, softcap: float = 0.0,
):
    """paged_attention_prefill's semantics on the split-KV kernel for a few
    new query rows per sequence over a long cache (attention_append.hip):
    head_dim 128, G in {1, 2, 4, 8}, bf16 or e5m2 cache; a window, a softcap
    or any other shape is a RuntimeError. q may be a row-strided view of the
    fused qkv output. n_splits = 0 takes _C.append_plan's split count
    (1..16 forces one)."""
    if q.is_cuda:
        _require_ext()
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _C.paged_attention_append(
            out, q, k_cache, v_cache, block_tables, query_start_loc, seq_lens,
            scale, n_splits, window, softcap
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


def paged_attention_prefill(
    q, k_cache, v_cache, block_tables, query_start_loc, seq_lens, scale: float,
    out=None, window: int = 0, softcap: float = 0.0,
):
    if q.is_cuda:
        _require_ext()
        if append_attn() and _C.append_plan(
            q.shape[0], seq_lens.shape[0], q.shape[1], k_cache.shape[1],
            q.shape[2], block_tables.shape[1], window, softcap
        )[0]:
            return paged_attention_append(
                q, k_cache, v_cache, block_tables, query_start_loc, seq_lens,
                scale, out=out,
            )
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


def dequant_workspace(device, N: int, K: int):
    """bf16 [N, K] view of the process-wide dequant workspace (the one
    int4_reserve_workspace grows). Never allocates: a weight reserves its
    size when it is built or moved."""
    ws = _INT4_WORKSPACE.get(torch.device(device))
    if ws is None or ws.numel() < N * K:
        raise RuntimeError(
            f"dequant workspace was not reserved for a [{N}, {K}] weight "
            f"on {device}"
        )
    return ws[: N * K].view(N, K)


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
    dense = int4_dequant(w, out=dequant_workspace(x.device, w.N, w.K))
    return torch.nn.functional.linear(x, dense)


# ---------------- MXFP4 (W4A8, OCP microscaling FP4 weights) ----------------
# `w` below is an engine.quant_mxfp4.Mxfp4Weight (packed qp/sp + N, K).

# Largest M the scaled-MFMA kernel serves; above it Mxfp4Linear runs
# mxfp4_dequant + the library GEMM and the decoder layers leave the fused
# branch. See docs/kernels.md for how it is set.
MXFP4_M_FUSED = 64


def mxfp4_m_max() -> int:
    """Largest M the scaled-MFMA kernels serve: MXFP4_M_FUSED, or
    KUBEAI_MXFP4_TILED_M where that is larger. Steps of MXFP4_M_FUSED < M <=
    mxfp4_m_max() run the output-tiled kernel (mxfp4_gemm_tiled) and keep the
    decoder layers in their fused-fp8 branch. Read at call time; unset, no
    route moves. See docs/kernels.md for the recommended value."""
    return max(MXFP4_M_FUSED, int(os.environ.get("KUBEAI_MXFP4_TILED_M", "0")))


def mxfp4_dequant(w, out=None):
    """Packed MXFP4 weight -> bf16 [N, K], bit-identical to w.dequant()."""
    if not w.qp.is_cuda:
        res = w.dequant()
        if out is not None:
            out.copy_(res)
            return out
        return res
    _require_ext()
    if out is None:
        out = torch.empty((w.N, w.K), dtype=torch.bfloat16, device=w.qp.device)
    _C.mxfp4_dequant(out, w.qp, w.sp, w.N, w.K)
    return out


def mxfp4_linear(xq, xs, w):
    """y[m, n] = bf16(acc[m, n] * xs[m]), acc the fp32 sum over k of the exact
    products xq[m, k] * w.dequant()[n, k]: bf16 [M, N]. xq is e4m3 [M, K] with
    16-byte aligned rows, xs its fp32 row scales [M] or [M, 1], 1 <= M <=
    mxfp4_m_max(). One launch on GPU, and a row's bytes do not depend on the
    rows around it: up to MXFP4_M_FUSED rows mxfp4_gemm (eight K-split
    partials summed in wave order), above it mxfp4_gemm_tiled (one accumulator
    per output over all of K). The two kernels agree with the exact product
    wherever fp32 summation is exact, not bit for bit elsewhere."""
    if not xq.is_cuda:
        acc = xq.float() @ w.dequant().float().t()
        return (acc * xs.reshape(-1, 1).float()).to(torch.bfloat16)
    _require_ext()
    M = xq.shape[0]
    if M > mxfp4_m_max():
        raise RuntimeError(
            f"mxfp4_linear takes at most {mxfp4_m_max()} rows, got {M}"
        )
    y = torch.empty((M, w.N), dtype=torch.bfloat16, device=xq.device)
    if M <= MXFP4_M_FUSED:
        _C.mxfp4_gemm(y, xq, xs, w.qp, w.sp, w.N, w.K)
    else:
        _C.mxfp4_gemm_tiled(y, xq, xs, w.qp, w.sp, w.N, w.K)
    return y


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


# ---------------- batched multi-LoRA apply, routed on the device ------------
# `table` below is an engine.lora.LoraTable: the device table of one (target,
# layer)'s adapter addresses, its host copy and the tensors it points at.


def lora_batched_t() -> int:
    """Largest T for which LoRAManager.apply takes lora_apply:
    KUBEAI_LORA_BATCHED_T, 64 when unset, at most 64; 0 keeps the per-adapter
    sgmv loop (and with it eager decode) at every T. Read at call time: the
    tests and A/B runs flip it."""
    try:
        limit = int(os.environ.get("KUBEAI_LORA_BATCHED_T", "64"))
    except ValueError:
        return 64
    return max(0, min(limit, 64))


def lora_vpart(device, T: int = 64) -> torch.Tensor:
    """Workspace one lora_apply needs at most: fp32 [32 splits, T, 64]."""
    return torch.empty(32 * T * 64, dtype=torch.float32, device=device)


def lora_apply(y, x, slots, table, vpart=None, ks: int = 0) -> None:
    """In place, for every row t with s = slots[t] >= 1 and rank R_s > 0:
    y[t] = bf16(float(y[t]) + B_s vb[t]), vb[t] = bf16(scale_s * A_s x[t]).
    All adapters of the batch in two launches on GPU; rows of slot 0 and of
    empty slots are never written. slots is int32 [T], T <= 64, x [T, K] with
    K % 8 == 0, y [T, N] with N % 16 == 0, ranks multiples of 8 up to 64.
    vpart (lora_vpart) must be passed where nothing may be allocated, as under
    graph capture; ks overrides the K split of _C.lora_plan."""
    if not x.is_cuda:
        ref.lora_apply(y, x, slots, table.rows)
        return
    _require_ext()
    if x.dim() == 2 and (x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16):
        x = x.contiguous()
    if vpart is None:
        vpart = lora_vpart(x.device, x.shape[0])
    _C.lora_apply(y, x, slots, table.dev, table.host, vpart, ks)


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


def empty_sample_result(B: int, device) -> SampleResult:
    """Buffers for greedy_sample_logprob(out=...): a decode graph keeps one
    set, so that its first node can read the tokens of the replay before."""
    packed = torch.zeros(2 * B, dtype=torch.int64, device=device)
    f = packed[B:].view(torch.float32)
    return SampleResult(packed[:B], f[:B], f[B:], packed)


def greedy_sample_logprob(logits, out: SampleResult | None = None) -> SampleResult:
    """greedy_sample's token, plus its log-probability and the row's
    logsumexp. On GPU the sampler's own two launches produce all three.
    out: write into these buffers (empty_sample_result) and return them."""
    if logits.is_cuda:
        _require_ext()
        res = out if out is not None else _empty_sample_result(logits)
        _C.greedy_sample_logprob(res.tokens, res.logprob, res.lse, logits)
        return res
    res = SampleResult(*ref.greedy_sample_logprob(logits))
    if out is None:
        return res
    for dst, src in zip(out[:3], res[:3]):
        dst.copy_(src)
    return out


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


def decode_advance(input_ids, positions, slots, seq_lens, block_tables,
                   n_blocks, b_live, tokens, block_size: int) -> None:
    """In place: a pure-decode step's inputs become the next step's (the
    sampled token at the next position and its slot from the block table),
    for rows below b_live[0] whose next position has a block; every other row
    stays as it is (ref.decode_advance). One launch, no host value read: the
    last node of a self-feeding decode graph."""
    if input_ids.is_cuda:
        _require_ext()
        _C.decode_advance(input_ids, positions, slots, seq_lens, block_tables,
                          n_blocks, b_live, tokens, block_size)
        return
    ref.decode_advance(input_ids, positions, slots, seq_lens, block_tables,
                       n_blocks, b_live, tokens, block_size)


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
